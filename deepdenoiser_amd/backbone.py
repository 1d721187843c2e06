"""The core architectures, recorded on a Graph: U-Net (reference TensorFlow/UNet.py) and Tiramisu (Tiramisu.py).

build(arch, g, x, namer) -> the backbone outputs, coarsest scale first (one output without multi-scale predictions).  Layers are created
through the namer in the reference's order: parameter creation order is the TensorFlow variable order."""


class Namer:
    """tf.layers auto-naming inside a variable scope: conv2d, conv2d_1, ...."""

    def __init__(self, scope):
        self.scope, self.counts = scope, {}

    def __call__(self, kind):
        n = self.counts.get(kind, 0)
        self.counts[kind] = n + 1
        return "%s/%s" % (self.scope, kind if n == 0 else "%s_%d" % (kind, n))


def build(arch, g, x, namer):
    return (unet if arch.core_name == "U-Net" else tiramisu)(arch, g, x, namer)


def unet(arch, g, x, namer):
    """UNet.predict (UNet.py:61-99); skip concats are channel ranges of one buffer per level."""
    filters, n = arch.filters, arch.convs_per_block
    steps = len(filters) - 1
    for f in filters:
        if f % 8:
            raise ValueError("U-Net filter counts must be multiples of 8 (got %s)" % (filters,))
    cats, results = [], []

    def conv_run(x, f, count, last_out=None, first_split=None):
        """`count` 3x3 convs + ReLU in a row (UNet.py:38-48)."""
        layers = [g.layer(namer("conv2d"), 3, x.C if c == 0 else f, f) for c in range(count)]
        for c, layer in enumerate(layers):
            x = g.conv(x, layer, relu=True, out=last_out if c == count - 1 else None, split_at=first_split if c == 0 else None)
        return x

    for i in range(steps):
        f = filters[i]
        cat = g.tensor(x.B, x.H, x.W, 2 * f, relu=True)
        x = conv_run(x, f, n, last_out=cat.view(0, f))
        cats.append(cat)
        x = g.maxpool(x, 3, 2)
    for i in range(steps):
        index = steps - i
        f = filters[index]
        # the first conv of an up level reads the skip concat of the level below ([skip | upsampled], f channels each)
        x = conv_run(x, f, n, first_split=f if i > 0 else None)
        if arch.use_multiscale_predictions:
            results.append(x)
        cat, fp = cats[index - 1], filters[index - 1]
        g.conv_transpose2(x, g.layer(namer("conv2d_transpose"), 2, x.C, fp, "convT2"), out=cat.view(fp, fp), relu=True)
        x = cat
    x = conv_run(x, filters[0], n, first_split=filters[0])
    results.append(x)
    return results


def tiramisu(arch, g, x, namer):
    """Tiramisu.predict (Tiramisu.py:67-111).  Each level owns ONE buffer laid out
    [down dense block | transpose-conv output | up dense growth]; every conv appends its channels in place, so the
    reference's per-conv tf.concat copies (Tiramisu.py:40) vanish."""
    filters, n = arch.filters, arch.convs_per_block
    steps = len(filters) - 1
    for f in filters:
        if f % 8:
            raise ValueError("Tiramisu filter counts must be multiples of 8 (got %s)" % (filters,))
    # channel bookkeeping per level
    c_in = [0] * (steps + 1)      # channels entering the level's down dense block
    c_down = [0] * (steps + 1)    # after the down dense block
    c = filters[0]
    for i in range(steps + 1):
        c_in[i] = c
        c = c + n * filters[i]
        c_down[i] = c
    total = [0] * (steps + 1)
    total[steps] = c_down[steps]
    for i in range(steps):
        total[i] = c_down[i] + filters[i] + n * filters[i]
    bufs = [g.tensor(x.B, x.H >> i, x.W >> i, total[i], relu=False) for i in range(steps + 1)]
    for b in bufs:
        b.gstate["zero_init"] = True

    def dense(buf, c0, f):
        return g.dense_block(buf, c0, f, [g.layer(namer("conv2d"), 3, c0 + j * f, f) for j in range(n)])

    pre = bufs[0].view(0, filters[0], relu=False)
    pre.self_mask = True
    g.conv(x, g.layer(namer("conv2d"), 3, x.C, filters[0]), relu=True, out=pre)
    pre.relu = False
    results = []
    for i in range(steps):
        cc = dense(bufs[i], c_in[i], filters[i])
        assert cc == c_down[i]
        t = g.conv(bufs[i].view(0, cc), g.layer(namer("conv2d"), 1, cc, cc), relu=False, in_relu=True)
        g.maxpool(t, 2, 2, out=bufs[i + 1].view(0, cc, relu=False))
    cc = dense(bufs[steps], c_in[steps], filters[steps])
    cur = bufs[steps].view(0, cc)
    for i in range(steps):
        index = steps - i
        if arch.use_multiscale_predictions:
            results.append(cur)
        lvl = index - 1
        fp = filters[lvl]
        up = bufs[lvl].view(c_down[lvl], fp, relu=False)
        up.self_mask = True
        g.conv_transpose3(cur, g.layer(namer("conv2d_transpose"), 3, cur.C, fp, "convT3"), out=up, relu=True)
        up.relu = False
        cc = dense(bufs[lvl], c_down[lvl] + fp, fp)
        cur = bufs[lvl].view(0, cc)
    results.append(cur)
    return results
