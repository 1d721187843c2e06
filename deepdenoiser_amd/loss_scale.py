"""Loss scaling of the optimisation step (include/dd_hip.h "dynamic loss scaling", csrc/dd_loss_scale.hip).

`Architecture(loss_scale=...)` takes
    None            the static default of the storage type (4096 for f16, 1 for bf16 / f32)
    a number        a static scale, baked into the launches (program.Program)
    "dynamic"       a scale that lives in device memory: halved when a step's gradients held an inf / NaN (the step is skipped), doubled after
                    `growth_interval` applied steps in a row
    a dict          "dynamic" with settings of its own: any of DEFAULTS' keys, e.g. {"init": 65536.0, "growth_interval": 2000}

The dynamic mode keeps the whole decision on the device (LossScaler): the scale, the skip, and the Adam step counter -- which advances only on
applied steps, so the host cannot know it without waiting -- are one dd_scaler_state record the kernels read and write.  A step issues three
launches (non-finite scan of the gradient arena, the guarded Adam update, the update of the record) and no device-to-host copy.
"""
import ctypes as C

import torch

from . import _lib as L

# init None: 65536 for f16 storage (gradients of a mean loss sit around 1e-7...1e-5 and fp16 flushes below 6e-8: start high, back off),
# 1 for bf16 / f32 (fp32 exponent range: nothing to rescue, and a scale of 1 multiplies exactly)
DEFAULTS = {"init": None, "growth": 2.0, "backoff": 0.5, "growth_interval": 2000, "min_scale": 1.0, "max_scale": float(2 ** 24)}
FIELDS = tuple(name for name, _ in L.ScalerState._fields_)


def is_dynamic(setting):
    return isinstance(setting, dict) or setting == "dynamic"


def parse(setting, dtype):
    """The settings of a dynamic scale as a complete dict (DEFAULTS filled in, `init` resolved for the storage type); None for a static one
    (None or a number: program.Program keeps handling those).  Raises ValueError for anything else."""
    if setting is None or (isinstance(setting, (int, float)) and not isinstance(setting, bool)):
        return None
    if not is_dynamic(setting):
        raise ValueError("loss_scale must be None, a positive number, 'dynamic' or a dict of dynamic settings (got %r)" % (setting,))
    cfg = dict(DEFAULTS)
    if isinstance(setting, dict):
        unknown = sorted(set(setting) - set(DEFAULTS))
        if unknown:
            raise ValueError("loss_scale: unknown setting(s) %s (known: %s)" % (", ".join(unknown), ", ".join(DEFAULTS)))
        cfg.update(setting)
    if cfg["init"] is None:
        cfg["init"] = 65536.0 if dtype == "f16" else 1.0
    cfg["growth_interval"] = int(cfg["growth_interval"])
    for k in ("init", "growth", "backoff", "min_scale", "max_scale"):
        cfg[k] = float(cfg[k])
    if not (cfg["init"] > 0.0 and cfg["growth"] >= 1.0 and 0.0 < cfg["backoff"] <= 1.0 and cfg["growth_interval"] > 0
            and 0.0 < cfg["min_scale"] <= cfg["max_scale"]):
        raise ValueError("loss_scale: need init > 0, growth >= 1, 0 < backoff <= 1, growth_interval > 0 and 0 < min_scale <= max_scale (got %r)" % (cfg,))
    return cfg


def cli_value(text):
    """argparse type of `--loss_scale {dynamic,<number>}`."""
    if text == "dynamic":
        return text
    try:
        value = float(text)
    except ValueError:
        value = 0.0
    if not (0.0 < value < float("inf")):
        import argparse
        raise argparse.ArgumentTypeError("'dynamic' or a positive number, not %r" % text)
    return value


class LossScaler:
    """The device-resident dd_scaler_state of one optimizer and the three launches of its step.  The initial scale is taken as given (not
    clamped to min_scale / max_scale: the clamps apply when the scale changes).  state() / scale() / skipped_steps copy the record to the
    host, which waits for the stream; nothing else here does."""

    def __init__(self, config, device, adam_t=0):
        self.config = dict(config)
        self.lib = L.load()
        assert C.sizeof(L.ScalerState) == 4 * len(FIELDS)
        self._words = torch.zeros(len(FIELDS), dtype=torch.int32, device=device)      # the record: 4-byte words in FIELDS order
        self.set_state({"scale": self.config["init"], "adam_t": int(adam_t)})

    @property
    def ptr(self):
        """Device address of the record == of its first word, the scale (what the *_dscale loss launches read)."""
        return self._words.data_ptr()

    def set_state(self, values):
        """Overwrite fields of the record (a dict by field name; stream-ordered, no wait)."""
        for k in values:
            if k not in FIELDS:
                raise KeyError(k)
        if "scale" in values:
            if not float(values["scale"]) > 0.0:
                raise ValueError("the loss scale must be positive")
            self._words[:1].view(torch.float32).fill_(float(values["scale"]))
        for i, k in enumerate(FIELDS):
            if k != "scale" and k in values:
                self._words[i:i + 1].fill_(int(values[k]))

    def state(self):
        """The record as a dict (waits for the stream)."""
        host = self._words.cpu()
        out = {k: int(host[i]) for i, k in enumerate(FIELDS)}
        out["scale"] = float(host[:1].view(torch.float32)[0])
        return out

    def scale(self):
        return self.state()["scale"]

    @property
    def skipped_steps(self):
        return self.state()["skipped_total"]

    def step(self, ps, lr, grad_scale, beta1, beta2, eps, stream, clipper=None):
        """Scan -> guarded Adam -> record update on `stream`, over the flat arenas of the ParamStore `ps`.  With a grad_clip.GradientClipper its
        two reduction launches run between the scan and the Adam launch (they divide by the scale the update is about to change), and the
        Adam launch multiplies by the coefficient they left on the device."""
        lib, n, c = self.lib, ps.values.numel(), self.config
        L.check(lib.dd_grads_nonfinite(ps.grads.data_ptr(), n, self.ptr, stream))
        if clipper is not None:
            clipper.measure(grad_scale, stream, scaler_ptr=self.ptr)
            L.check(lib.dd_adam_step_scaled_clipped(ps.values.data_ptr(), ps.grads.data_ptr(), ps.m.data_ptr(), ps.v.data_ptr(), n, lr, beta1, beta2,
                                                    eps, grad_scale, self.ptr, clipper.ptr, stream))
        else:
            L.check(lib.dd_adam_step_scaled(ps.values.data_ptr(), ps.grads.data_ptr(), ps.m.data_ptr(), ps.v.data_ptr(), n, lr, beta1, beta2, eps,
                                            grad_scale, self.ptr, stream))
        L.check(lib.dd_scaler_update(self.ptr, c["growth"], c["backoff"], c["growth_interval"], c["min_scale"], c["max_scale"], stream))
