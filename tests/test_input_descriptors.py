"""What the input assembly asks its kernels to do: the dd_assemble_input table (tile and frame mode), the dd_gather_input table of
DD_FUSE_INPUT=0 and the one-launch decision of the embedding gradient, field by field against expectations worked out here from the
architecture JSON -- SourceEncoder's order (members, auxiliary features, feature flags; SourceEncoder.py:29-79) and 3 + variance channels per
pass restated in this file, not taken from deepdenoiser_amd/input_assembly.py.  Every pointer is checked as an offset into the buffer it must
lie in.  Built on the CPU device from the cross-compiled library; nothing is launched."""
import ctypes as C
import math

import pytest
import torch

from deepdenoiser_amd import _lib as L
from deepdenoiser_amd import configs
from deepdenoiser_amd.architecture import Architecture
from deepdenoiser_amd.input_assembly import write_constant_flags
from deepdenoiser_amd.naming import Naming
from deepdenoiser_amd.render_passes import RenderPasses

SMALL = dict(filters=(16, 16), convs=1)
B, H, W = 2, 16, 32
# name: (architecture, dtype)
CASES = {
    "example": (configs.architecture(**SMALL), "bf16"),
    "combined_one_hot": (configs.architecture(tuple_type="COMBINED", flag_mode="ONE_HOT_ENCODING", **SMALL), "f32"),
    "no_flags": (configs.architecture(flag_mode="NONE", **SMALL), "bf16"),
    "raw_kp_source": (configs.architecture(standardized_kp_source=False, **SMALL), "bf16"),
    "misaligned_embedding": (configs.architecture(variance=False, auxiliary={}, **SMALL), "bf16"),
}
FP_FIELDS = [k for k, _ in L.FeatureParams._fields_]


def _f32(x):
    return C.c_float(x).value


def _pass(name, channels, j):
    """A pass as the expectation sees it: name, source channels, its feature_variance / standardization JSON."""
    return dict(name=name, cs=channels, var=j["feature_variance"], std=j["standardization"])


def _variance_channels(p):
    return 0 if not p["var"]["use_variance"] else 1 if p["var"]["compress_to_one_channel"] else p["cs"]


def _fp(p):
    v, s = p["var"], p["std"]
    return [int(s["use_log1p"]), _f32(s["mean"]), _f32(1.0 / math.sqrt(s["variance"])), int(v["use_variance"]),
            int(v["compute_before_standardization"]), int(v["variance_mode"] == "neighbor"), int(v["relative_variance"]),
            int(v["compress_to_one_channel"]), _f32(1e-4)]


def _expected(aj):
    """(tuples [(name, member passes)], auxiliary passes, flag mode, sorted flag names) of an architecture JSON (Architecture.py:367-473:
    combined names sorted, Color / Direct / Indirect inside; a SINGLE tuple per loaded pass, a COMBINED one per combined feature with its
    generated passes)."""
    se = aj["architecture"]["source_encoder"]
    tuples = []
    for cname in sorted(aj["combined_features"]):
        members = []
        for ftype in ("Color", "Direct", "Indirect"):
            fname = aj["combined_features"][cname][ftype]
            p = _pass(fname or cname + " " + ftype, RenderPasses.number_of_channels(fname), aj["combined_features_handling"][ftype])
            if se["feature_prediction_tuple_type"] == "SINGLE":
                if fname:
                    tuples.append((fname, [p]))
            else:
                members.append(p)
        if members:
            tuples.append((cname, members))
    aux = [_pass(n, aj["auxiliary_features"][n]["number_of_channels"], aj["auxiliary_features"][n]) for n in sorted(aj["auxiliary_features"])]
    return tuples, aux, se["feature_flag_mode"], sorted(n for n, _ in tuples)


def _build(case, monkeypatch, fuse=True, dtype=None):
    if fuse:
        monkeypatch.delenv("DD_FUSE_INPUT", raising=False)
    else:
        monkeypatch.setenv("DD_FUSE_INPUT", "0")
    aj, dt = CASES[case]
    arch = Architecture(aj, device="cpu", dtype=dtype or dt, seed=2)
    return aj, arch, arch.program(B, H, W, training_json=configs.training())


def _embedding_ptr(arch, row, D):
    p = [p for p in arch.params.params if p.name == "embedding/feature_flags_embedding_matrix"][0]
    return arch.params.values.data_ptr() + 4 * p.offset + row * D * 4


def _expected_entries(aj, arch, prog):
    """Per tuple the expected entries as dictionaries: kind, nch, dst_ch and, for a pass, p / head (index in head order or None) / plane (its
    plane of the DD_FUSE_INPUT=0 staging buffer); for the flags, src."""
    tuples, aux, mode, names = _expected(aj)
    T, M, V = len(tuples), len(tuples[0][1]), len(names)
    NF = T * M
    out = []
    for t, (tname, members) in enumerate(tuples):
        entries, ch = [], 0
        for p, head in [(p, j * T + t) for j, p in enumerate(members)] + [(p, None) for p in aux]:
            nch = 3 + _variance_channels(p)
            entries.append(dict(kind=0, p=p, head=head, plane=head if head is not None else NF + aux.index(p), nch=nch, dst_ch=ch))
            ch += nch
        if mode == "ONE_HOT_ENCODING":
            entries.append(dict(kind=2, nch=V, dst_ch=ch, src=prog.flags_raw[tname].data_ptr()))
            ch += V
        elif mode == "EMBEDDING":
            entries.append(dict(kind=1, nch=V // 2, dst_ch=ch, src=_embedding_ptr(arch, names.index(tname), V // 2)))
            ch += V // 2
        assert ch == arch.input_channels(), tname
        out.append(entries)
    VL = 3 + max(_variance_channels(p) for _, members in tuples for p in members + aux)
    return out, VL, NF, len(aux)


def _check_assemble(tab, expected, VL, prog, frames=None):
    n = len(expected[0])
    assert len(tab) == len(expected) * n
    plane = B * H * W * VL * 4
    for t, entries in enumerate(expected):
        for e, x in enumerate(entries):
            en, where = tab[t * n + e], (t, e)
            assert (en.kind, en.nch, en.dst_ch) == (x["kind"], x["nch"], x["dst_ch"]), where
            if x["kind"] != 0:
                assert en.src == x["src"] and (en.cs, en.std_out, en.ld_std) == (0, None, 0), where
                continue
            p = x["p"]
            assert en.src == (prog.raw if frames is None else frames)[p["name"]].data_ptr() and en.cs == p["cs"], where
            assert [getattr(en.fp, k) for k in FP_FIELDS] == _fp(p), where
            if x["head"] is not None:
                assert (en.std_out, en.ld_std) == (prog.sources.data_ptr() + x["head"] * plane, VL), where
            else:
                assert (en.std_out, en.ld_std) == (None, 0), where
        assert tab[t * n + n - 1].dst_ch + tab[t * n + n - 1].nch == prog.arch.input_channels(), t


def _input_launches(prog):
    """The launches at the head of the forward list that carry the input-assembly tag."""
    n = 0
    while n < len(prog.g.fwd_ops) and getattr(prog.g.fwd_ops[n], "tag", None) == "input_assembly":
        n += 1
    assert not any(getattr(op, "tag", None) == "input_assembly" for op in prog.g.fwd_ops[n:])
    return n


@pytest.mark.parametrize("case", list(CASES))
def test_assemble_table_tile_and_frame_mode(lib, monkeypatch, case):
    aj, arch, prog = _build(case, monkeypatch)
    expected, VL, NF, NA = _expected_entries(aj, arch, prog)
    assert prog.fused_input and prog.VL == VL and tuple(prog.sources.shape) == (NF * B, H, W, VL)
    assert (prog.X.B, prog.X.C) == (len(expected) * B, arch.input_channels())
    kp_raw = not aj["architecture"]["kernel_prediction"]["use_standardized_source_for_kernel_prediction"]
    assert (prog.raw3 is not None) == kp_raw and (not kp_raw or tuple(prog.raw3.shape) == (NF * B, H, W, 3))
    assert _input_launches(prog) == (NF if kp_raw else 0) + 1      # raw3's identity prepares, then the one assembly launch
    tile = prog.input.fill_assemble_table()
    _check_assemble(tile, expected, VL, prog)
    # frame mode: only the pass entries' sources change, to the frames
    frames = {x["p"]["name"]: torch.zeros(24, 40, x["p"]["cs"]) for entries in expected for x in entries if x["kind"] == 0}
    frame = prog.input.fill_assemble_table(frames)
    _check_assemble(frame, expected, VL, prog, frames)
    patched = type(tile).from_buffer_copy(tile)
    for i, x in enumerate(x for entries in expected for x in entries):
        if x["kind"] == 0:
            patched[i].src = frames[x["p"]["name"]].data_ptr()
    assert bytes(patched) == bytes(frame)


def test_observed_layouts(lib, monkeypatch):
    """The layouts of the cases in numbers: tuples, entries per tuple, channels."""
    for case, T, widths, ld in (("example", 17, [4, 4, 8], 16), ("combined_one_hot", 8, [4, 4, 4, 4, 8], 24), ("no_flags", 17, [4, 4], 8),
                                ("misaligned_embedding", 17, [3, 8], 16)):
        aj, arch, prog = _build(case, monkeypatch)
        tab = prog.input.fill_assemble_table()
        n = len(widths)
        assert len(tab) == T * n and [tab[i].nch for i in range(n)] == widths, case
        assert (arch.input_channels(), prog.X.ld) == (sum(widths), ld), case
    # (the misaligned case: one 3-channel pass, the embedding row at channel 3 of 11)
    assert (tab[0].kind, tab[0].nch, tab[1].kind, tab[1].dst_ch) == (0, 3, 1, 3)


@pytest.mark.parametrize("case", list(CASES))
def test_unfused_gather_table(lib, monkeypatch, case):
    aj, arch, prog = _build(case, monkeypatch, fuse=False)
    expected, VL, NF, NA = _expected_entries(aj, arch, prog)
    assert not prog.fused_input and tuple(prog.sources.shape) == ((NF + NA) * B, H, W, VL)
    # one prepare launch per pass, raw3's identity prepares, the one gather launch
    assert _input_launches(prog) == (NF + NA) + (NF if prog.raw3 is not None else 0) + 1
    tab = prog.input.fill_gather_table()
    n = len(expected[0])
    assert len(tab) == len(expected) * n
    for t, entries in enumerate(expected):
        for e, x in enumerate(entries):
            en = tab[t * n + e]
            got = (en.src, en.pixel_stride, en.batch_stride_pixels, en.nch, en.dst_ch)
            if x["kind"] == 0:
                assert got == (prog.sources.data_ptr() + x["plane"] * B * H * W * VL * 4, VL, H * W, x["nch"], x["dst_ch"]), (t, e)
            elif x["kind"] == 2:
                assert got == (x["src"], x["nch"], H * W, x["nch"], x["dst_ch"]), (t, e)
            else:
                assert got == (x["src"], 0, 0, x["nch"], x["dst_ch"]), (t, e)
    with pytest.raises(RuntimeError):
        prog.enable_frame_input(24, 40)


@pytest.mark.parametrize("case,dtype,one_launch", [("example", "bf16", True), ("example", "f32", True),
                                                   ("misaligned_embedding", "f32", False), ("misaligned_embedding", "bf16", False)])
def test_embedding_gradient_one_launch_decision(lib, monkeypatch, case, dtype, one_launch):
    """dd_colsum_segments reads whole 16-byte vectors from the embedding's first channel: taken when emb_ch0 * esz is a multiple of 16 (the
    example: channel 8), not at channel 3 (3 * 4 and 3 * 2 bytes), where one dd_colsum per tuple runs."""
    aj, arch, prog = _build(case, monkeypatch, dtype=dtype)
    expected, _, _, _ = _expected_entries(aj, arch, prog)
    emb_ch0, esz = expected[0][-1]["dst_ch"], 4 if dtype == "f32" else 2
    assert expected[0][-1]["kind"] == 1 and ((emb_ch0 * esz) % 16 == 0) == one_launch
    assert prog.input.emb_ch0 == emb_ch0 and prog.input.embedding_one_launch() == one_launch
    assert sum(1 for op in prog.g.bwd_ops if prog.input.emb in getattr(op, "grad_params", ())) == 1


def test_constant_one_hot_planes(lib, monkeypatch):
    aj, arch, prog = _build("combined_one_hot", monkeypatch)
    tuples, aux, _, names = _expected(aj)
    for tname, _ in tuples:      # exactly one 1.0 per pixel, at the tuple's index among the sorted names
        buf = torch.full((B, H, W, len(names)), 7.0)
        write_constant_flags(arch, tname, buf)
        want = torch.zeros(len(names))
        want[names.index(tname)] = 1.0
        assert torch.equal(buf, want.expand(B, H, W, len(names)))
    # set_inputs: a caller's feature_flag/<name> tensor is copied, every other tuple gets the constant plane
    gen = torch.Generator().manual_seed(0)
    feats = {Naming.source_feature_name(p["name"], index=0): torch.rand(B, H, W, p["cs"], generator=gen)
             for p in [p for _, members in tuples for p in members] + aux}
    given = torch.rand(B, H, W, len(names), generator=gen)
    feats[Naming.feature_flags_name(tuples[1][0])] = given
    for buf in prog.flags_raw.values():
        buf.fill_(7.0)
    prog.set_inputs(feats)
    for t, (tname, members) in enumerate(tuples):
        want = torch.zeros(len(names))
        want[names.index(tname)] = 1.0
        assert torch.equal(prog.flags_raw[tname], given if t == 1 else want.expand(B, H, W, len(names))), tname
        for p in members + aux:
            assert torch.equal(prog.raw[p["name"]], feats[Naming.source_feature_name(p["name"], index=0)]), p["name"]
