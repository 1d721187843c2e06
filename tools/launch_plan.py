"""The launch plan of one built program as text, for diffing two trees without a GPU (the program is built on the CPU device, nothing runs):
    python tools/launch_plan.py [cfg2|tiramisu] [bf16|f32|f16] [train|infer] [B] [H] [W]
One line per launch of the four lists (list, tag, function, info, gradient parameters, kept buffers), one per pack record, then the parameter
names in creation order.  The DD_* switches are read when the program is built, so they are set in the environment of the call."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from deepdenoiser_amd import configs  # noqa: E402
from deepdenoiser_amd.architecture import Architecture  # noqa: E402


def _buffers(keep):
    """The tensors of a launch's `keep` (nested tuples / lists, None for an absent operand), flattened in order."""
    if isinstance(keep, torch.Tensor):
        return ["%s:%s" % ("x".join(str(n) for n in keep.shape), str(keep.dtype).replace("torch.", ""))]
    if isinstance(keep, (tuple, list)):
        return [b for k in keep for b in _buffers(k)]
    return []


def describe(prog):
    """The lines of the plan of a built Program."""
    g = prog.g
    lines = []
    for name, ops in (("pack", g.pack_ops), ("label", prog.label_ops), ("fwd", g.fwd_ops), ("bwd", g.bwd_ops)):
        for op in ops:
            lines.append("%s %s %s info=%s grads=%s keep=%s" % (
                name, getattr(op, "tag", None), getattr(op, "__name__", type(op).__name__),
                json.dumps(getattr(op, "info", None), sort_keys=True, default=str),
                ",".join(p.name for p in getattr(op, "grad_params", ())), " ".join(_buffers(getattr(op, "keep", None)))))
    for rec in g._pack_records:
        lines.append("packrec %s %s" % (rec[0].name, " ".join(str(v) for v in rec[2:])))
    lines += ["param %s" % p.name for p in g.params.params]
    return lines


def main(argv):
    which, dtype, mode = (argv + ["cfg2", "bf16", "train"][len(argv):])[:3]
    B, H, W = (int(v) for v in (argv[3:6] + ["2", "64", "64"][len(argv[3:6]):]))
    aj = configs.cfg2_unet_kpcn() if which == "cfg2" else configs.cfg3_tiramisu(filters=(16, 24, 32), convs=2)
    arch = Architecture(aj, device="cpu", dtype=dtype, seed=2)
    prog = arch.program(B, H, W, training_json=configs.bench_training() if mode == "train" else None)
    print("\n".join(describe(prog)))


if __name__ == "__main__":
    main(sys.argv[1:])
