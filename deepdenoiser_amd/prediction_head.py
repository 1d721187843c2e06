"""From the backbone outputs to the predictions of every scale, recorded on a Graph (Architecture.predict, reference
TensorFlow/Architecture.py:573-600): the 1x1 post-processing and the kernel prediction (or the direct prediction) of every scale, the
multi-scale compose net (MultiScalePrediction.py) and the inverse standardization.

Every builder decides its lowering first and records only the launches that will run: a fused launch takes the place of the layer-wise ones
by being queued instead of them, never by taking recorded launches out of the lists again."""
import ctypes as C
import math
import os

import torch

from . import _lib as L
from .engine import DT
from .loss_desc import block_ptr


def head_tensor(device, N, h, w, requires_grad=True):
    """An fp32 tensor of N 3-channel images: the layout of predictions, kernel-prediction sources and targets."""
    buf = torch.zeros((N, h, w, 3), dtype=torch.float32, device=device)
    return DT(buf, N, h, w, 3, 3, 0, "f32", False, requires_grad)


def avgpool_op(lib, x, y, f):
    def run(stream):
        L.check(lib.dd_avgpool(x.ptr, x.ld, y.ptr, y.ld, 3, x.B, x.H, x.W, f, stream))
    return run


class PredictionHead:
    """The head builders of one program over `head`, the features in head order (f' = j*T + t: member-major, every member's block of T*B
    images is contiguous)."""

    def __init__(self, arch, g, B, head, training):
        self.arch, self.g, self.lib, self.B, self.head, self.training = arch, g, g.lib, B, head, training
        self.T, self.M = len(arch.feature_prediction_tuples), arch.tuple_size
        self.post_hidden = []          # hidden activations of the layer-wise head's first 1x1 conv, per scale (tools/debug_grads.py)
        self.loss_inverts = {}         # scale -> (standardized prediction, groups): the inversions that dd_loss_head runs itself (invert)
        self.compose_scratch = []      # scratch of the streaming compose backward (earlier buffers stay alive: bound launches point at them)

    # ================================================================== 1x1 post-processing + kernel prediction of every scale
    def predict(self, outs, namer, sources, dims):
        """outs: the backbone outputs, coarsest first; sources: the [N, H, W, 3] fp32 buffer the predicted kernels are applied to; dims: (h, w) of
        every scale.  -> the (standardized) predictions, finest scale first."""
        arch, g = self.arch, self.g
        M, oc = self.M, arch.number_of_output_channels
        # bf16 / fp16 storage, one tuple member, 3x3 or 5x5 kernels: the 1x1 -> ReLU -> 1x1 -> softmax -> filter-apply chain of a scale is ONE
        # launch each way (csrc/dd_head.hip); the K-channel hid / logits tensors and their gradients never exist in HBM
        fuse_head = (arch.use_kernel_prediction and M == 1 and arch.kernel_size in (3, 5) and g.dtype != "f32"
                     and all(o.C % 8 == 0 and o.C <= 128 for o in outs) and os.environ.get("DD_FUSE_HEAD", "1") != "0")
        self.fused_head = fuse_head
        post, head_layers, hidden = [], [], []
        for o in outs:     # coarsest first: variable creation order (Architecture.py:573-575)
            la, lb = g.layer(namer("conv2d"), 1, o.C, oc), g.layer(namer("conv2d"), 1, oc, oc)
            head_layers.append((o, la, lb))
            if not fuse_head:
                hid = g.conv(o, la, relu=True)
                self.post_hidden.append(hid)
                hidden.append((hid, lb))
                post.append(g.conv(hid, lb, relu=False))
        if arch.use_multiscale_predictions:
            post, head_layers, hidden = list(reversed(post)), list(reversed(head_layers)), list(reversed(hidden))
        self.post = post
        # Layer-wise head of a half-precision program: the kernel-prediction launches compute their logits in fp32 from `hid` and the fp32 master
        # weights of the second 1x1 layer (dd_kpcn_hidden_*) instead of reading the bf16 / fp16 logits that layer stored -- its tensor remains for
        # the layer's weight / data gradient launches, which consume d logits as before.  DD_KPCN_FP32_LOGITS=0: the round-3 behaviour.
        self.fp32_logits = (not fuse_head and g.dtype != "f32" and arch.use_kernel_prediction and os.environ.get("DD_KPCN_FP32_LOGITS", "1") != "0")

        N = len(self.head) * self.B
        assert len(dims) == len(head_layers)
        K = [head_tensor(self.arch.device, N, h, w) for (h, w) in dims]
        if not arch.use_kernel_prediction:
            for s in range(len(post)):
                self._direct(post[s], K[s])
            return K
        src0 = DT(sources, N, dims[0][0], dims[0][1], 3, 3, 0, "f32")
        srcs = []
        for s, (h, w) in enumerate(dims):
            if s == 0:
                src = src0
            else:
                src = head_tensor(self.arch.device, N, h, w, requires_grad=False)
                g.fwd(avgpool_op(self.lib, src0, src, 1 << s))
            srcs.append(src)
            if not fuse_head:
                self._kpcn(src, post[s], K[s], hidden[s] if self.fp32_logits else None)
        if fuse_head:
            # the head launches go in variable-creation order of their layers (coarsest first), like the 1x1 convs they replace:
            # the reverse program then reaches the finest scale's backbone output first, as before
            for s in reversed(range(len(dims))):
                self._kpcn_head(head_layers[s], srcs[s], K[s])
        return K

    def _kpcn(self, src, logits, out, hidden=None):
        """KernelPredictor.predict (Architecture.py:260-289) + KernelPrediction.kernel_prediction.
        hidden = (hid, layer): the logits are computed in the launch, in fp32, from the second 1x1 layer's input and master weights."""
        g, lib, arch = self.g, self.lib, self.arch
        k2, ks = arch.kernel_size ** 2, arch.kernel_size
        TB, M = self.T * self.B, self.M
        esz = 4 if g.dtype == "f32" else 2
        h, w = out.H, out.W
        hid, lb = hidden if hidden is not None else (None, None)

        def hidden_args(j):      # (parameter pointers exist once ParamStore.finalize() has run: evaluated at launch / capture time)
            return (hid.ptr, hid.ld, hid.C, g.params.value_ptr(lb.kernel) + 4 * j * k2, lb.cout, g.params.value_ptr(lb.bias) + 4 * j * k2)

        def run(stream):
            for j in range(M):
                if hid is not None:
                    L.check(lib.dd_kpcn_hidden_fwd(block_ptr(src, j * TB), src.ld, *hidden_args(j), block_ptr(out, j * TB), out.ld, TB, h, w, ks, g.code, stream))
                    continue
                L.check(lib.dd_kpcn_fwd(block_ptr(src, j * TB), src.ld, logits.ptr + j * k2 * esz, logits.ld,
                                        block_ptr(out, j * TB), out.ld, TB, h, w, ks, g.code, stream))
        g.fwd(run, "kpcn_apply")

        def backward():
            if not out.grad_written:
                return
            go, gl = out.grad(), logits.grad()

            def runb(stream):
                for j in range(M):
                    pad = (logits.Cp - j * k2) if j == M - 1 else k2
                    if hid is not None:
                        L.check(lib.dd_kpcn_hidden_bwd(block_ptr(src, j * TB), src.ld, *hidden_args(j), block_ptr(go, j * TB), go.ld,
                                                       gl.ptr + j * k2 * esz, gl.ld, pad, TB, h, w, ks, g.code, stream))
                        continue
                    L.check(lib.dd_kpcn_bwd(block_ptr(src, j * TB), src.ld, logits.ptr + j * k2 * esz, logits.ld,
                                            block_ptr(go, j * TB), go.ld, gl.ptr + j * k2 * esz, gl.ld, pad, TB, h, w, ks, g.code, stream))
            g.bwd(runb, "kpcn_apply")
            logits.mark_grad_written()
        g.on_backward(backward)

    def _kpcn_head(self, head, src, out):
        """AdjustNumberOfChannels.predict + KernelPredictor.predict of one scale (Architecture.py:237-244, 260-289) as one launch each way."""
        g, lib = self.g, self.lib
        x, la, lb = head
        assert x.B == out.B and (x.H, x.W) == (out.H, out.W)

        def make():
            ha = L.HeadArgs()
            self._head_args(ha, head, src, out)

            def run(stream, ha=ha):
                L.check(lib.dd_kpcn_head_fwd(C.byref(ha), stream))
            return run
        g.fwd(g._defer(make, "kpcn_head", keep=(x.buf, src.buf, out.buf)))

        def backward():
            if not (out.grad_written and x.requires_grad):
                return
            go, gx = out.grad(), x.grad()
            desc = (head, src, out, go, gx, 1 if x.grad_written else 0)

            def makeb():
                hb = L.HeadArgs()
                self._head_args(hb, *desc)

                def runb(stream, hb=hb):
                    L.check(lib.dd_kpcn_head_bwd(C.byref(hb), stream))
                return runb
            # (head_bwd: consecutive scales run as one launch, merge_backward)
            g.bwd(g._defer(makeb, "kpcn_head", keep=(go.buf, gx.buf), head_bwd=desc), grad_params=[la.kernel, la.bias, lb.kernel, lb.bias])
            x.mark_grad_written()
        g.on_backward(backward)

    def _head_args(self, h, head, src, out, go=None, gx=None, accumulate=0):
        """Fills the dd_kpcn_head_fwd arguments `h` of one scale; with go / gx (d out, d x) also what dd_kpcn_head_bwd adds to them."""
        ps = self.g.params
        x, la, lb = head
        h.x, h.ldx, h.C, h.src, h.ldsrc = x.ptr, x.ld, x.C, src.ptr, src.ld
        h.wa, h.ba, h.wb, h.bb = ps.value_ptr(la.kernel), ps.value_ptr(la.bias), ps.value_ptr(lb.kernel), ps.value_ptr(lb.bias)
        h.out, h.ld_out = out.ptr, out.ld
        h.N, h.H, h.W, h.ksize, h.dtype = x.B, x.H, x.W, self.arch.kernel_size, self.g.code
        if go is not None:
            h.dout, h.ld_dout, h.dx, h.ld_dx, h.accumulate_dx = go.ptr, go.ld, gx.ptr, gx.ld, accumulate
            h.dwa, h.dba, h.dwb, h.dbb = ps.grad_ptr(la.kernel), ps.grad_ptr(la.bias), ps.grad_ptr(lb.kernel), ps.grad_ptr(lb.bias)

    def merge_backward(self):
        """The head backward launches of the scales -- consecutive in the reverse program, independent of each other -- as ONE launch
        (dd_kpcn_head_bwd_multi): the coarse scales are mostly fixed cost (DD_HEAD_BWD_MULTI=0 keeps them apart)."""
        g, lib = self.g, self.lib
        if os.environ.get("DD_HEAD_BWD_MULTI", "1") == "0":
            return
        ops, out, i = g.bwd_ops, [], 0
        while i < len(ops):
            j = i
            while j < len(ops) and getattr(ops[j], "head_bwd", None) is not None and j - i < 3:
                j += 1
            if j - i < 2:
                out.append(ops[i])
                i += 1
                continue
            members = ops[i:j]

            def make(descs=[op.head_bwd for op in members]):
                arr = (L.HeadArgs * len(descs))()
                for h, desc in zip(arr, descs):
                    self._head_args(h, *desc)

                def run(stream, arr=arr, n=len(descs)):
                    L.check(lib.dd_kpcn_head_bwd_multi(arr, n, stream))
                return run
            out.append(g._defer(make, "kpcn_head", grad_params=tuple(p_ for op in members for p_ in op.grad_params),
                                keep=[getattr(op, "keep", None) for op in members]))
            i = j
        g.bwd_ops = out

    def _direct(self, logits, out):
        """No kernel prediction: the 3 output channels of each tuple member are the prediction (Architecture.py:520-522)."""
        g, lib = self.g, self.lib
        TB, M = self.T * self.B, self.M
        esz = 4 if g.dtype == "f32" else 2
        npix = TB * out.H * out.W

        def run(stream):
            for j in range(M):
                L.check(lib.dd_convert_channels(logits.ptr + j * 3 * esz, g.code, logits.ld, block_ptr(out, j * TB), L.DD_F32, 3, 3, 3, npix, stream))
        g.fwd(run)

        def backward():
            if not out.grad_written:
                return
            go, gl = out.grad(), logits.grad()

            def runb(stream):
                for j in range(M):
                    pad = (logits.Cp - j * 3) if j == M - 1 else 3
                    L.check(lib.dd_convert_channels(block_ptr(go, j * TB), L.DD_F32, 3, gl.ptr + j * 3 * esz, g.code, gl.ld, 3, pad, npix, stream))
            g.bwd(runb)
            logits.mark_grad_written()
        g.on_backward(backward)

    # ================================================================== inverse standardization
    def invert(self, s, x, in_loss_head=False):
        """FeaturePrediction.prediction_invert_standardization (Architecture.py:134-138) of scale s, grouped by identical parameters.
        in_loss_head: dd_loss_head runs the inversion and its gradient itself (loss_desc.loss_plan, fuse_invert): the inverted tensor is
        allocated, (x, groups) kept in loss_inverts[s] for the loss build, and nothing is queued."""
        g, lib, B = self.g, self.lib, self.B
        groups = []
        for i, f in enumerate(self.head):
            st = f.feature_standardization
            key = (st.use_log1p, st.mean, st.variance) if f.invert_standardization else (False, 0.0, 1.0)
            if groups and groups[-1][0] == key:
                groups[-1][2] += 1
            else:
                groups.append([key, i, 1])
        if all(k[0] == (False, 0.0, 1.0) for k in groups):
            return x
        y = head_tensor(self.arch.device, x.B, x.H, x.W)
        if in_loss_head:
            self.loss_inverts[s] = (x, groups)
            return y
        per = B * x.H * x.W * 3

        def run(stream):
            for (log1p, mean, var), i0, cnt in groups:
                L.check(lib.dd_invert_std_fwd(block_ptr(x, i0 * B), block_ptr(y, i0 * B), per * cnt, int(log1p), mean, math.sqrt(var), stream))
        g.fwd(run)

        def backward():
            if not y.grad_written:
                return
            gy, gx = y.grad(), x.grad()
            assert not x.grad_written, "invert-standardization is expected to be the first gradient writer"

            def runb(stream):
                for (log1p, mean, var), i0, cnt in groups:
                    L.check(lib.dd_invert_std_bwd(block_ptr(x, i0 * B), block_ptr(gy, i0 * B), block_ptr(gx, i0 * B), per * cnt,
                                                  int(log1p), mean, math.sqrt(var), stream))
            g.bwd(runb)
            x.mark_grad_written()
        g.on_backward(backward)
        return y

    # ================================================================== multi-scale compose net
    def compose(self, small, fine, namer):
        """MultiScalePrediction.compose_scales (MultiScalePrediction.py:36-93): pack -> 1x1 -> two residual blocks of 3x3 -> 1x1 -> blend, in
        one of three lowerings chosen before anything is recorded.  Layer-wise (f32 storage, or DD_FUSE_COMPOSE=0): eight forward launches and
        their reverse launches.  Fused forward, layer-wise backward (training with DD_FUSE_COMPOSE_BWD=0): ONE forward launch that keeps the
        24-channel frames in LDS (csrc/dd_compose.hip) and stores what the layer-wise backward reads into its tensors (acts[1] and acts[3] as
        relu(r): identical as masks and as in_relu operands).  Fully fused (inference, and training by default): one launch each way; a
        training program keeps the activations and the blend weight, an inference program nothing."""
        g = self.g
        # parameter creation order is the TensorFlow variable order, whatever the lowering
        layers = [g.layer(namer("conv2d"), k, cin, cout) for k, cin, cout in ((1, 6, 24), (3, 24, 24), (3, 24, 24), (3, 24, 24), (3, 24, 24), (1, 24, 1))]
        fuse_fwd = g.dtype != "f32" and os.environ.get("DD_FUSE_COMPOSE", "1") != "0"
        fuse_bwd = fuse_fwd and (not self.training or os.environ.get("DD_FUSE_COMPOSE_BWD", "1") != "0")
        if not fuse_bwd:
            out, netin, acts, wl = self._compose_layerwise(small, fine, layers, no_forward=fuse_fwd)
            if fuse_fwd:
                g.fwd(self._compose_fwd(small, fine, out, layers, netin, acts, wl))
            return out
        N, h, w = fine.B, fine.H, fine.W
        out = head_tensor(self.arch.device, N, h, w)
        acts, wl = [], None
        if self.training:
            acts, wl = [g.tensor(N, h, w, 24) for _ in range(5)], g.tensor(N, h, w, 1)
        g.fwd(self._compose_fwd(small, fine, out, layers, None, acts, wl))      # (the fused backward rebuilds the packed net input itself)
        if self.training:
            self._compose_bwd(small, fine, out, layers, acts, wl)
        return out

    def _compose_layerwise(self, small, fine, layers, no_forward):
        """The compose net layer by layer.  no_forward: only the reverse program is recorded (the fused forward launch stores what it reads).
        -> (out, packed input, the five activations, blend weight)"""
        g, lib = self.g, self.lib
        N, h, w = fine.B, fine.H, fine.W
        lay_in, lay_res, lay_out = layers[0], layers[1:5], layers[5]
        netin = g.tensor(N, h, w, 6, requires_grad=self.training)

        def pack(stream):
            L.check(lib.dd_compose_pack(small.ptr, small.ld, fine.ptr, fine.ld, netin.ptr, netin.ld, netin.Cp, N, h, w, g.code, stream))
        if not no_forward:
            g.fwd(pack)

        def pack_backward():
            if not netin.grad_written:
                return
            gn, gs, gf = netin.grad(), small.grad(), fine.grad()

            def runb(stream):
                L.check(lib.dd_compose_unpack_bwd(gn.ptr, gn.ld, gs.ptr, gs.ld, gf.ptr, gf.ld, N, h, w, g.code, stream))
            g.bwd(runb)
        g.on_backward(pack_backward)

        x = g.conv(netin, lay_in, relu=True, no_forward=no_forward)
        acts = [x]
        for la, lb in (lay_res[:2], lay_res[2:]):
            r = g.conv(x, la, relu=False, in_relu=True, no_forward=no_forward)
            x = g.conv(r, lb, relu=False, in_relu=True, res=x, no_forward=no_forward)
            acts += [r, x]
        wl = g.conv(x, lay_out, relu=True, no_forward=no_forward)
        out = head_tensor(self.arch.device, N, h, w)

        def blend(stream):
            L.check(lib.dd_compose_blend_fwd(small.ptr, small.ld, fine.ptr, fine.ld, wl.ptr, wl.ld, out.ptr, out.ld, N, h, w, g.code, stream))
        if not no_forward:
            g.fwd(blend)

        def blend_backward():
            if not out.grad_written:
                return
            go, gs, gf, gw = out.grad(), small.grad(), fine.grad(), wl.grad()
            acc_small = 1 if small.grad_written else 0
            assert not fine.grad_written

            def runb(stream):
                L.check(lib.dd_compose_blend_bwd(go.ptr, go.ld, small.ptr, small.ld, fine.ptr, fine.ld, wl.ptr, wl.ld,
                                                 gs.ptr, gs.ld, acc_small, gf.ptr, gf.ld, gw.ptr, gw.ld, gw.Cp, N, h, w, g.code, stream))
            g.bwd(runb)
            small.mark_grad_written()
            fine.mark_grad_written()
            wl.mark_grad_written()
        g.on_backward(blend_backward)
        return out, netin, acts, wl

    def _compose_fwd(self, small, fine, out, layers, netin, acts, wl):
        """The fused forward launch (dd_compose_net_fwd).  netin / acts / wl: where it stores the packed input, the five activations and the
        blend weight for a backward; None / empty: not stored."""
        g, lib, ps = self.g, self.lib, self.g.params
        lay_in, lay_res, lay_out = layers[0], layers[1:5], layers[5]

        def make_fused():
            ca = L.ComposeArgs()
            ca.small, ca.ld_small, ca.fine, ca.ld_fine, ca.out, ca.ld_out = small.ptr, small.ld, fine.ptr, fine.ld, out.ptr, out.ld
            ca.w_in, ca.b_in = ps.value_ptr(lay_in.kernel), ps.value_ptr(lay_in.bias)
            for i, lay in enumerate(lay_res):
                ca.w_res[i], ca.b_res[i] = ps.value_ptr(lay.kernel), ps.value_ptr(lay.bias)
            ca.w_out, ca.b_out = ps.value_ptr(lay_out.kernel), ps.value_ptr(lay_out.bias)
            if netin is not None:
                ca.save_netin, ca.ld_netin = netin.ptr, netin.ld
            for i, t in enumerate(acts):
                ca.save_act[i], ca.ld_act[i] = t.ptr, t.ld
            if wl is not None:
                ca.save_wl, ca.ld_wl = wl.ptr, wl.ld
            ca.N, ca.H, ca.W, ca.dtype = fine.B, fine.H, fine.W, g.code

            def fused(stream, ca=ca):
                L.check(lib.dd_compose_net_fwd(C.byref(ca), stream))
            return fused
        return g._defer(make_fused, "compose_net", keep=(small.buf, fine.buf, out.buf, [t.buf for t in (netin, wl) if t is not None],
                                                         [t.buf for t in acts]))

    def _compose_bwd(self, small, fine, out, layers, acts, wl):
        """The fused backward (dd_compose_net_bwd) as one tape entry: blend, six data gradients, six weight gradients and the unpack."""
        g, lib, ps = self.g, self.lib, self.g.params
        N, h, w = fine.B, fine.H, fine.W
        lay_in, lay_res, lay_out = layers[0], layers[1:5], layers[5]

        def fused_backward():
            if not out.grad_written:
                return
            go, gs, gf = out.grad(), small.grad(), fine.grad()
            acc_small = 1 if small.grad_written else 0
            assert not fine.grad_written
            cb = L.ComposeBwdArgs()
            cb.small, cb.ld_small, cb.fine, cb.ld_fine, cb.dout, cb.ld_dout = small.ptr, small.ld, fine.ptr, fine.ld, go.ptr, go.ld
            for i, t in enumerate(acts):
                cb.act[i], cb.ld_act[i] = t.ptr, t.ld
            cb.wl, cb.ld_wl = wl.ptr, wl.ld
            cb.d_small, cb.ld_dsmall, cb.accumulate_small, cb.d_fine, cb.ld_dfine = gs.ptr, gs.ld, acc_small, gf.ptr, gf.ld
            cb.N, cb.H, cb.W, cb.dtype = N, h, w, g.code
            if os.environ.get("DD_COMPOSE_STREAM_BWD", "1") != "0":
                # scratch of the two row-streaming launches (the parked gradient tensors): one buffer per program, shared by the scale
                # transitions (they run one after the other)
                need = int(lib.dd_compose_bwd_scratch_bytes(N, h, w))
                pool = self.compose_scratch
                if not pool or pool[-1].numel() < need:
                    pool.append(torch.empty(need, dtype=torch.uint8, device=self.arch.device))
                cb.scratch, cb.scratch_bytes = pool[-1].data_ptr(), pool[-1].numel()

            def make_fused_bwd():
                cb.w_in, cb.w_out = ps.value_ptr(lay_in.kernel), ps.value_ptr(lay_out.kernel)
                cb.dw_in, cb.db_in = ps.grad_ptr(lay_in.kernel), ps.grad_ptr(lay_in.bias)
                cb.dw_out, cb.db_out = ps.grad_ptr(lay_out.kernel), ps.grad_ptr(lay_out.bias)
                for i, lay in enumerate(lay_res):
                    cb.w_res[i], cb.dw_res[i], cb.db_res[i] = ps.value_ptr(lay.kernel), ps.grad_ptr(lay.kernel), ps.grad_ptr(lay.bias)

                def runb(stream, cb=cb):
                    L.check(lib.dd_compose_net_bwd(C.byref(cb), stream))
                return runb
            g.bwd(g._defer(make_fused_bwd, "compose_net", keep=(go.buf, gs.buf, gf.buf)),
                  grad_params=[p_ for lay in layers for p_ in (lay.kernel, lay.bias)])
            small.mark_grad_written()
            fine.mark_grad_written()
        g.on_backward(fused_backward)
