"""Gradient clipping by global norm and per-variable norms (include/dd_hip.h "gradient clipping", csrc/dd_grad_norm.hip): the middle of the
usual scale -> unscale -> clip -> step sequence, the reference's missing `tf.clip_by_global_norm`.

`Architecture(clip_norm=...)` takes
    None            off: the optimisation step issues the launches it always did
    a number > 0    the gradients are multiplied by  clip_norm / max(global norm, clip_norm)  in the Adam launch
and `Architecture(track_gradient_norms=True)` asks for the measurement alone (coef stays 1).

One segmented reduction over the flat gradient arena (and the value arena at the same indices) gives the global norm, the coefficient and
every variable's gradient norm, weight norm and count of inf / NaN gradient elements: two launches in front of the Adam launch, on its stream.
The coefficient stays in device memory, where the Adam launch reads it: a step makes no device-to-host copy.  `report()` copies the tables
to the host, which waits for the stream, like LossScaler.state(); nothing else here does.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L

CHUNK = L.GRAD_CHUNK


def parse(setting):
    """The clip norm as a float, None for off.  Raises ValueError for anything but None or a positive finite number."""
    if setting is None:
        return None
    if isinstance(setting, bool) or not isinstance(setting, (int, float)) or not (0.0 < float(setting) < float("inf")):
        raise ValueError("clip_norm must be None or a positive finite number (got %r)" % (setting,))
    return float(setting)


def cli_value(text):
    """argparse type of `--clip_norm X`: a finite number >= 0 (0: off)."""
    try:
        value = float(text)
    except ValueError:
        value = -1.0
    if not (0.0 <= value < float("inf")):
        import argparse
        raise argparse.ArgumentTypeError("a finite number >= 0 (0: off), not %r" % text)
    return value


def resolve_clip_norm(cli, training_json):
    """What `Architecture(clip_norm=...)` gets: the command line's --clip_norm when given, else Training.json's optional "gradient_clip_norm".
    Absent, null or 0 means off (None), on either side: `--clip_norm 0` switches a clip norm of the JSON off."""
    value = cli if cli is not None else training_json.get("gradient_clip_norm")
    if value is None or (isinstance(value, (int, float)) and not isinstance(value, bool) and value == 0):
        return None
    return parse(value)


def plan_chunks(params, chunk=CHUNK):
    """The chunk table of dd_grad_norms.  Pure integer logic (CPU-testable).

    params: [(name, offset, size)] layout of the flat arenas (variable-creation order; the words between offset + size and the next offset
            are padding)
    Returns (chunks, var_first): chunks = [(offset, length, variable index)], every variable cut in order into pieces of at most `chunk`
    elements -- no piece spans two variables or touches a padding word; var_first[v] : var_first[v + 1] are the chunks of variable v."""
    chunks, var_first = [], [0]
    for v, (_, offset, size) in enumerate(params):
        offset, size = int(offset), int(size)
        if offset < 0 or size < 0:
            raise ValueError("variable %d: offset %d, size %d" % (v, offset, size))
        for lo in range(0, size, chunk):
            chunks.append((offset + lo, min(chunk, size - lo), v))
        var_first.append(len(chunks))
    return chunks, var_first


class GradientClipper:
    """The device tables of one optimizer's arenas (chunk table, per-chunk partial records, per-variable norms, the clip record) and the two
    launches of dd_grad_norms.  `ptr` is the device address of the dd_grad_clip record the *_clipped Adam launches read."""

    def __init__(self, params, grads, values, clip_norm=None):
        """params: [(name, offset, size)] of the arenas `grads` and `values` (flat fp32 device tensors of one length)."""
        self.lib = L.load()
        self.clip_norm = parse(clip_norm)
        self.names = [name for name, _, _ in params]
        self.grads, self.values = grads, values
        assert grads.dtype == values.dtype == torch.float32 and grads.numel() == values.numel() and grads.device == values.device
        chunks, var_first = plan_chunks(params)
        if not chunks or any(b == a for a, b in zip(var_first, var_first[1:])):
            raise ValueError("every variable needs at least one element")
        if max(o + n for o, n, _ in chunks) > grads.numel():
            raise ValueError("a variable lies outside the arena of %d elements" % grads.numel())
        assert C.sizeof(L.GradChunk) == 16 and C.sizeof(L.GradVarNorms) == 24 and C.sizeof(L.GradClip) == 20
        table = np.zeros(len(chunks), dtype=[("offset", "<i8"), ("length", "<i4"), ("variable", "<i4")])
        table["offset"], table["length"], table["variable"] = (np.array(c, dtype=np.int64) for c in zip(*chunks))
        dev = grads.device
        self.n_chunks, self.n_vars = len(chunks), len(params)
        self._chunks = torch.from_numpy(table.view(np.int32)).to(dev)
        self._var_first = torch.tensor(var_first, dtype=torch.int32, device=dev)
        self._partials = torch.zeros(self.n_chunks * L.GRAD_PARTIAL_BYTES // 4, dtype=torch.int32, device=dev)
        self._var_norms = torch.zeros(self.n_vars * 6, dtype=torch.int32, device=dev)      # dd_grad_var_norms rows as 4-byte words
        self._clip = torch.zeros(5, dtype=torch.int32, device=dev)                         # the dd_grad_clip record
        self._clip[1:2].view(torch.float32).fill_(1.0)                                    # (coef of a record no launch has written yet)

    @classmethod
    def for_store(cls, ps, clip_norm=None):
        """Over the arenas of an engine.ParamStore."""
        return cls([(p.name, p.offset, p.size) for p in ps.params], ps.grads, ps.values, clip_norm)

    @property
    def ptr(self):
        return self._clip.data_ptr()

    def measure(self, grad_scale, stream, scaler_ptr=None):
        """The two reduction launches on `stream`.  The factor of the true gradient is `grad_scale` (what dd_adam_step is given), or -- with the
        device address of a dd_scaler_state -- grad_scale / st->scale (what dd_adam_step_scaled computes)."""
        L.check(self.lib.dd_grad_norms(self.grads.data_ptr(), self.values.data_ptr(), self._chunks.data_ptr(), self.n_chunks,
                                       self._var_first.data_ptr(), self.n_vars, self._partials.data_ptr(), self._var_norms.data_ptr(), self.ptr,
                                       self.clip_norm or 0.0, grad_scale, scaler_ptr, stream))

    def tables(self):
        """(per-variable table, clip record) as the bytes the device holds (waits for the stream)."""
        return self._var_norms.cpu().numpy().tobytes(), self._clip.cpu().numpy().tobytes()

    def report(self):
        """What the last measure() found (waits for the stream): {"grad_norm", "coef", "grad_factor", "nonfinite_variables", "nonfinite_total",
        "variables": {name: {"grad_norm", "weight_norm", "nonfinite", "grad_sq", "weight_sq"}}}.  The norms are those of the TRUE gradient
        (the stored one times grad_factor); grad_sq / weight_sq are the device's sums of squares of the stored values."""
        rows, rec = self.tables()
        rec = L.GradClip.from_buffer_copy(rec)
        rows = np.frombuffer(rows, dtype=[("grad_sq", "<f8"), ("weight_sq", "<f8"), ("nonfinite", "<u4"), ("reserved", "<u4")])
        factor = abs(float(rec.grad_factor))
        variables = {}
        for name, r in zip(self.names, rows):
            variables[name] = {"grad_norm": factor * math.sqrt(float(r["grad_sq"])), "weight_norm": math.sqrt(float(r["weight_sq"])),
                               "nonfinite": int(r["nonfinite"]), "grad_sq": float(r["grad_sq"]), "weight_sq": float(r["weight_sq"])}
        return {"grad_norm": float(rec.grad_norm), "coef": float(rec.coef), "grad_factor": float(rec.grad_factor),
                "nonfinite_variables": int(rec.nonfinite_variables), "nonfinite_total": int(rec.nonfinite_total), "variables": variables}
