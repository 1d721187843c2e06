"""What the op-level conv tests share (tests/test_gpu_conv_bwd_ops.py, tests/test_gpu_conv_fwd_ops.py): operands as channel views inside
sentinel-filled wider buffers, fp32 outputs between guard words, dd_pack_weights checked bit for bit, and the elementwise gate."""
import torch

import conv_bwd_ref as R
from deepdenoiser_amd import _lib as L
from gpu_util import gate

SENTINEL = 12288.0      # exact in fp32, bf16 and fp16
G = 4                   # guard words before and after an fp32 array (16 bytes: the arrays stay 16-byte aligned)
DT = {"bf16": (L.DD_BF16, torch.bfloat16), "f16": (L.DD_F16, torch.float16), "f32": (L.DD_F32, torch.float32), "f32full": (L.DD_F32, torch.float32)}


def stream():
    return torch.cuda.current_stream().cuda_stream


class View:
    """[B, H, W, C] values as channels [off, off + C) of a buffer of row length ld: channels up to `cv` zero, every other channel the sentinel."""

    def __init__(self, shape, C_, cv, ld, off, dtype, values=None, pad=0.0):
        self.C, self.cv, self.ld, self.off = C_, cv, ld, off
        self.buf = torch.full(tuple(shape) + (ld,), SENTINEL, dtype=DT[dtype][1], device="cuda")
        self.buf[..., off + C_:off + cv] = pad
        if values is not None:
            self.buf[..., off:off + C_] = values.to(DT[dtype][1]).cuda()
        self.before = self.buf.clone()

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.off * self.buf.element_size()

    def values(self):
        return self.buf[..., self.off:self.off + self.C].double().cpu()

    def pads(self):
        return self.buf[..., self.off + self.C:self.off + self.cv].double().cpu()

    def neighbours_intact(self):
        return bool((self.buf[..., :self.off] == SENTINEL).all()) and bool((self.buf[..., self.off + self.cv:] == SENTINEL).all())

    def unchanged(self):
        return torch.equal(self.buf.view(torch.uint8), self.before.view(torch.uint8))


class Guarded:
    """n fp32 words (zero, or `values`) between G sentinel words on either side."""

    def __init__(self, n, values=None):
        self.n = n
        self.buf = torch.full((n + 2 * G,), SENTINEL, dtype=torch.float32, device="cuda")
        self.buf[G:G + n] = 0.0 if values is None else values.float().reshape(-1).cuda()

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * G

    def values(self):
        return self.buf[G:G + self.n].double().cpu()

    def guards_intact(self):
        return bool((self.buf[:G] == SENTINEL).all()) and bool((self.buf[G + self.n:] == SENTINEL).all())


def bits(t):
    return t.contiguous().view(torch.int16)


def pack_image(lib, what, src, dtype, taps, n, k, n_pad, k_pad, st, sn, sk, flip):
    """dd_pack_weights of the flat fp32 master `src`; the image is compared bit for bit with the numpy restatement (padding exactly zero) and
    must end where it should.  Returns the device image."""
    src = src.float().contiguous().cuda()
    total = taps * n_pad * k_pad
    dst = torch.full((total + 8,), SENTINEL, dtype=DT[dtype][1], device="cuda")
    L.check(lib.dd_pack_weights(src.data_ptr(), dst.data_ptr(), DT[dtype][0], taps, n, k, n_pad, k_pad, st, sn, sk, flip, stream()))
    torch.cuda.synchronize()
    if DT[dtype][1] == torch.float32:      # f32 storage: the restatement without a rounding
        want = torch.zeros(taps, n_pad, k_pad)
        t, nn, kk = torch.meshgrid(torch.arange(taps), torch.arange(n), torch.arange(k), indexing="ij")
        want[:, :n, :k] = src.cpu()[((taps - 1 - t) if flip else t) * st + nn * sn + kk * sk]
        assert torch.equal(dst[:total].cpu().view(torch.int32), want.reshape(-1).view(torch.int32)), "dd_pack_weights %s %s: image differs from the restatement" % (what, dtype)
    else:
        want = R.pack_weights(src.cpu().numpy(), dtype, taps, n, k, n_pad, k_pad, st, sn, sk, flip)
        assert want.numel() == total
        assert torch.equal(bits(dst[:total].cpu()), bits(want)), "dd_pack_weights %s %s: image differs from the restatement" % (what, dtype)
    assert bool((dst[total:] == SENTINEL).all()), "dd_pack_weights wrote past its image"
    return dst


def pack(lib, kind, role, master, cin, cout, dtype):
    """dd_pack_weights with the strides and n_pad / k_pad rule of engine.Layer.packed(role).  Returns (device image, n_pad, k_pad)."""
    taps, n, k, st, sn, sk, flip = R.pack_params(kind, role, cin, cout)
    n_pad, k_pad = R.pack_dims(n, k)
    return pack_image(lib, "%s %s %dx%d" % (kind, role, cin, cout), master, dtype, taps, n, k, n_pad, k_pad, st, sn, sk, flip), n_pad, k_pad


def gated(name, got, ref, gate_t):
    got = got.double().cpu()
    assert tuple(got.shape) == tuple(ref.shape), (name, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), name + ": non-finite values"
    w = R.worst_ratio(got, ref, gate_t)
    print("%-84s worst error / gate %.3f over %d elements" % (name, w, ref.numel()))
    gate(name, w, 1.0)
    return w
