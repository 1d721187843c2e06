"""numpy float64 restatement of dd_grad_norms (include/dd_hip.h "gradient clipping"; tf.clip_by_global_norm) and the arena layouts its tests share.

    per variable    grad_sq = sum of squares of the FINITE stored gradient elements, weight_sq = sum of squares of the values, nonfinite = the
                    number of inf / NaN gradient elements (they add to no sum)
    global          grad_norm = |gs| * sqrt(sum of grad_sq), coef = clip_norm / max(grad_norm, clip_norm);  clip_norm <= 0 (or None): coef = 1;
                    any non-finite gradient element: coef = 1 and grad_norm = +inf
"""
import numpy as np

# the variable sizes of the issue: around one 16-byte vector, around one 4096-element chunk, two chunks + 3, and a run of 300 one-element variables
SIZES = [1, 3, 4, 5, 4095, 4096, 4097, 8195] + [1] * 300


def layout(sizes=SIZES, align=4):
    """[(name, offset, size)] with engine.ParamStore's alignment (every variable starts on a multiple of 4 elements = 16 bytes) and the total."""
    out, total = [], 0
    for i, n in enumerate(sizes):
        out.append(("v%d_%d" % (i, n), total, n))
        total += (n + align - 1) // align * align
    return out, max(total, 4)


def reference(params, grads, values, gs, clip_norm):
    """params: [(name, offset, size)]; grads, values: the float32 arenas (padding included, never read).  -> dict like GradientClipper.report()
    plus the float64 sums."""
    grads, values = np.asarray(grads, dtype=np.float32), np.asarray(values, dtype=np.float32)
    variables, total, bad_vars, bad = {}, 0.0, 0, 0
    for name, off, size in params:
        g, w = grads[off:off + size].astype(np.float64), values[off:off + size].astype(np.float64)
        finite = np.isfinite(g)
        gsq, wsq, nf = float(np.sum(g[finite] ** 2)), float(np.sum(w ** 2)), int(np.sum(~finite))
        variables[name] = {"grad_sq": gsq, "weight_sq": wsq, "nonfinite": nf, "grad_norm": abs(gs) * np.sqrt(gsq), "weight_norm": np.sqrt(wsq)}
        total += gsq
        bad += nf
        bad_vars += int(nf > 0)
    norm = abs(float(gs)) * np.sqrt(total)
    coef = 1.0
    if bad:
        norm = float("inf")
    elif clip_norm is not None and clip_norm > 0:
        coef = clip_norm / max(norm, clip_norm)
    return {"grad_norm": float(norm), "coef": float(coef), "grad_sq_total": total, "nonfinite_variables": bad_vars, "nonfinite_total": bad,
            "variables": variables}


def arenas(params, total, seed=3):
    """(grads, values) float32 arenas over `params`: values over many magnitudes (the draw of test_adam_tf_form), with +-3.4e38 (one each, so
    that the true norm at gs = 0.5 stays below FLT_MAX), denormals and +-0 planted in the gradients; every PADDING word of both is NaN."""
    rng = np.random.default_rng(seed)
    g = (rng.standard_normal(total) * np.exp(3 * rng.standard_normal(total))).astype(np.float32)
    w = (rng.standard_normal(total) * np.exp(rng.standard_normal(total))).astype(np.float32)
    by_size = {}
    for name, off, size in params:
        by_size.setdefault(size, off)
    g[by_size[4097] + 4096] = 3.4e38          # the element tail of a chunk
    g[by_size[8195] + 5000] = -3.4e38         # a 16-byte vector of the second chunk
    g[by_size[4095]:by_size[4095] + 8] = [0.0, -0.0, 1e-45, -1e-40, 1e-38, 0.0, -0.0, 1e-39]
    g[by_size[3]:by_size[3] + 3] = [1e-40, -0.0, 2.5]
    g[by_size[1]] = 1e-41                     # a one-element variable whose only gradient is a denormal
    covered = np.zeros(total, dtype=bool)
    for name, off, size in params:
        covered[off:off + size] = True
    g[~covered] = np.nan
    w[~covered] = np.nan
    return g, w
