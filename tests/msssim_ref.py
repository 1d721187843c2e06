"""Reference for the MS-SSIM loss term (test infrastructure; CPU, float64).

A restatement of tf.image.ssim_multiscale of TensorFlow 1.x as BaseFeatureTraining.ms_ssim calls it (Training.py:178-204):
max_val = 1, power_factors = (0.0448, 0.2856, 0.3001), filter_size 11, filter_sigma 1.5, k1 0.01, k2 0.03.  Written after TF's own
functions, in their order and form (image_ops_impl.py: _fspecial_gauss, _ssim_helper, _ssim_per_channel, ssim_multiscale):
the torch version uses an 11 x 11 DEPTHWISE conv2d (not the separable form the HIP kernels use), avg_pool2d(2), relu, pow and prod, so that
torch autograd gives the gradient oracle; the numpy version is an independent loop over windows (forward only).
PARITY UNPINNED against live TensorFlow, like the rest of the oracle (oracle/tf_ops.py).
"""
import numpy as np
import torch
import torch.nn.functional as F

POWER_FACTORS = (0.0448, 0.2856, 0.3001)
FILTER_SIZE, FILTER_SIGMA, K1, K2, MAX_VAL = 11, 1.5, 0.01, 0.03, 1.0


def fspecial_gauss(size=FILTER_SIZE, sigma=FILTER_SIGMA, dtype=torch.float64):
    """_fspecial_gauss: softmax over the size*size values -(i^2 + j^2) / (2 sigma^2)."""
    coords = torch.arange(size, dtype=dtype) - (size - 1) / 2.0
    g = coords ** 2 * (-0.5 / sigma ** 2)
    g = g.reshape(1, -1) + g.reshape(-1, 1)
    return torch.softmax(g.reshape(-1), dim=0).reshape(size, size)


def ssim_helper(x, y, reducer, max_val=MAX_VAL, compensation=1.0):
    """_ssim_helper: (luminance, contrast-structure) maps."""
    c1, c2 = (K1 * max_val) ** 2, (K2 * max_val) ** 2
    mean0, mean1 = reducer(x), reducer(y)
    num0 = mean0 * mean1 * 2.0
    den0 = mean0 ** 2 + mean1 ** 2
    luminance = (num0 + c1) / (den0 + c1)
    num1 = reducer(x * y) * 2.0
    den1 = reducer(x ** 2 + y ** 2)
    c2 = c2 * compensation
    cs = (num1 - num0 + c2) / (den1 - den0 + c2)
    return luminance, cs


def ssim_per_channel(x, y):
    """_ssim_per_channel on NHWC tensors: (ssim [B,C], cs [B,C]) = means over the VALID filter positions."""
    c = x.shape[3]
    kernel = fspecial_gauss(dtype=x.dtype).reshape(1, 1, FILTER_SIZE, FILTER_SIZE).repeat(c, 1, 1, 1)

    def reducer(t):      # depthwise_conv2d, strides 1, VALID
        return F.conv2d(t.permute(0, 3, 1, 2), kernel, groups=c).permute(0, 2, 3, 1)
    luminance, cs = ssim_helper(x, y, reducer)
    return (luminance * cs).mean(dim=(1, 2)), cs.mean(dim=(1, 2))


def ms_ssim_factors(x, y, power_factors=POWER_FACTORS):
    """The relu'd factors [B, C, levels] whose weighted product is MS: cs of every level but the last, ssim of the last (mcs.pop())."""
    mcs = []
    ssim = None
    for k in range(len(power_factors)):
        if k > 0:      # both tensors: 2x2 / stride-2 average pool (sides are even here: no symmetric pad)
            assert x.shape[1] % 2 == 0 and x.shape[2] % 2 == 0
            x = F.avg_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
            y = F.avg_pool2d(y.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
        assert min(x.shape[1], x.shape[2]) >= FILTER_SIZE, "level %d is smaller than the filter" % k
        ssim, cs = ssim_per_channel(x, y)
        mcs.append(torch.relu(cs))
    mcs.pop()
    return torch.stack(mcs + [torch.relu(ssim)], dim=-1)


def ms_ssim(x, y, power_factors=POWER_FACTORS):
    """tf.image.ssim_multiscale: [B] = mean over channels of prod_k factor_k ^ power_k."""
    f = ms_ssim_factors(x, y, power_factors)
    w = torch.tensor(power_factors, dtype=f.dtype)
    return torch.prod(f ** w, dim=-1).mean(dim=-1)


def ms_ssim_term(x, y, weight):
    """BaseFeatureTraining.loss, Training.py:231-232 + :203: weight * (1 - mean over images)."""
    return weight * (1.0 - ms_ssim(x, y).mean())


# ---------------------------------------------------------------------------------------------------------- independent numpy loops
def ms_ssim_numpy(x, y, power_factors=POWER_FACTORS):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = FILTER_SIZE
    e = np.array([[np.exp(-((i - 5) ** 2 + (j - 5) ** 2) / (2 * FILTER_SIGMA ** 2)) for j in range(n)] for i in range(n)])
    g = e / e.sum()
    c1, c2 = (K1 * MAX_VAL) ** 2, (K2 * MAX_VAL) ** 2
    B, _, _, C = x.shape
    out = np.zeros(B)
    for b in range(B):
        for c in range(C):
            px, py = x[b, :, :, c], y[b, :, :, c]
            ms = 1.0
            for k, power in enumerate(power_factors):
                if k > 0:
                    px = 0.25 * (px[0::2, 0::2] + px[0::2, 1::2] + px[1::2, 0::2] + px[1::2, 1::2])
                    py = 0.25 * (py[0::2, 0::2] + py[0::2, 1::2] + py[1::2, 0::2] + py[1::2, 1::2])
                h, w = px.shape
                cs_sum = ssim_sum = 0.0
                for i in range(h - n + 1):
                    for j in range(w - n + 1):
                        wx, wy = px[i:i + n, j:j + n], py[i:i + n, j:j + n]
                        mx, my = (g * wx).sum(), (g * wy).sum()
                        sxy, s2 = (g * wx * wy).sum(), (g * (wx * wx + wy * wy)).sum()
                        cs = (2 * sxy - 2 * mx * my + c2) / (s2 - mx * mx - my * my + c2)
                        lum = (2 * mx * my + c1) / (mx * mx + my * my + c1)
                        cs_sum += cs
                        ssim_sum += lum * cs
                cnt = (h - n + 1) * (w - n + 1)
                v = (ssim_sum if k == len(power_factors) - 1 else cs_sum) / cnt
                ms *= max(v, 0.0) ** power
            out[b] += ms / C
    return out


# ---------------------------------------------------------------------------------------------------------- whole-model oracle
def wrap_oracle(monkeypatch, record=None):
    """Teaches oracle.training._FT.loss the ms_ssim term for the duration of a test (the oracle itself is not edited): the original runs with
    the weight set to 0, then weight * (1 - mean ms_ssim(predicted[0], target[0])) is added -- once, without the multi-scale scale factor
    (Training.py:223-232).  `record`: a list that receives (name, factors [B,C,3]) of every evaluated term."""
    from oracle import training as OT
    original = OT._FT.loss

    def loss(self, multiscale):
        w = self.ssim_w
        self.ssim_w = 0.0
        try:
            result = original(self, multiscale)
        finally:
            self.ssim_w = w
        if w > 0:
            if record is not None:
                record.append((self.name, ms_ssim_factors(self.predicted[0], self.target[0]).detach()))
            result = result + ms_ssim_term(self.predicted[0], self.target[0], w)
        return result
    monkeypatch.setattr(OT._FT, "loss", loss)
