"""Importance-sampled training windows of resident frames (`train.py --frames_crops importance`): a window is drawn with a probability that
grows with how much the noisy source renderings differ from the target inside it.

A Monte-Carlo rendering is mostly easy -- flat walls, sky, converged diffuse regions where the source already equals the target -- and such a
window adds almost nothing to a SMAPE loss or its gradient.  The kernel-prediction denoiser this network descends from (KPCN) draws its
training patches from a density built on the frames for that reason; the reference cannot (TFRecordsCreator.py:125-133 fixes its tiles on
disk), a bank of resident frames can.

    cell      a G x G block of a scene, G a divisor of the tile T.  ONE dd_importance_cells launch (csrc/dd_frame_importance.hip) reads every
              sample of the colour passes that are both a source and a target once and gives per cell the sum of the loss's own SMAPE
              |s - t| / ((|s| + |t|) + 1e-2) (LossDifference.py:30-34) over pixels, channels, sources and passes; cells[s] is that sum divided
              by the number of terms: a mean SMAPE in [0, 1]
    window    the lattice windows of scene s have the origins (i G, j G), i <= (h - T) // G, j <= (w - T) // G; the weight W[s][i, j] is the sum
              of the (T / G)^2 cell means under the window (a float64 integral image)
    density   p = (1 - floor) W / sum(W over all scenes) + floor U,  U(s, i, j) = 1 / (n_scenes n_lattice(s)) -- what 'random' crops give a
              lattice window; the floor keeps easy regions from vanishing.  sum(W) = 0 (every source equals its target): p = U

The draw of one example, from the random.Random all ranks share (the ORDER of the calls is part of the contract: every rank replays it):

    u = rng.random();  the window is the first index with cdf > u * cdf[-1]  (cdf: the float64 running sum of p, scenes in order, row-major)
    y0 = min(i G + rng.randrange(G), h - T);  x0 = min(j G + rng.randrange(G), w - T)     (the jitter keeps every origin reachable; y0 // G = i)
    tup = index_tuples[rng.randrange(len(index_tuples))]

The scores are computed on the device because the planes live there; the draw stays on the host, like the two other crop modes.  The measure
is noise only: no structure term (target gradients, normals) and no loss re-weighting -- this is a deliberate change of the training
distribution, as in KPCN.

Refreshed from the running model (`--frames_importance_refresh N`, off by default): after a few epochs the windows worth drawing are the
ones the model still gets wrong.  The model's error of a cell is the mean SMAPE(prediction, target) with the same formula and epsilon as the
noise score, the mean SMAPE(source, target) -- a network that returns its input scores exactly the noise map -- so the refreshed map needs
no new unit:

    score     ONE dd_importance_update launch (csrc/dd_importance_update.hip) inside every training step, between the forward and the backward
              (Program.step_tail_ops: the backward may reuse prediction buffers), adds per cell that lies wholly inside an example's window
              llrint(mean 2^32) and 1 to two flat integer tables on the device (ImportanceScorer)
    fold      every N steps the tables are read, added over the ranks (an integer sum: exact) and zeroed; a visited cell moves towards the mean
              m of its visits, cells = (1 - rate) cells + rate m, every other cell keeps its bytes, and weights, total and cdf are rebuilt
              (ImportanceMap.fold).  The draw contract above is untouched.

Visited cells fall as the model learns, unvisited ones keep their noise score and grow relatively heavier until they are visited; the floor
keeps its role.  The refreshed map is not saved with a checkpoint: a resumed run starts from the noise map again."""
import ctypes as C

import numpy as np

EPSILON = 1e-2            # LossDifference.difference's default epsilon
DEFAULT_FLOOR = 0.25      # a choice, not a measured optimum
DEFAULT_RATE = 0.5        # of a refresh (ImportanceMap.fold): a choice as well

# dd_importance_cell as a numpy record (16 bytes)
CELL_DTYPE = np.dtype([("source_plane0", "<i4"), ("target_plane", "<i4"), ("y0", "<i4"), ("x0", "<i4")])


def colour_passes(bank):
    """The passes the scores are taken over: in both bank.source_channels and bank.target_channels with 3 channels, sorted by name."""
    names = sorted(n for n, ch in bank.source_channels.items() if ch == 3 and bank.target_channels.get(n) == 3)
    if not names:
        raise ValueError("importance crops: the frames give no colour pass that is both a source and a target")
    return names


def resolve_cell(tile, cell=None):
    """The cell side G: `cell`, or the largest of 16, 8, 4, 2, 1 that divides the tile."""
    tile = int(tile)
    if cell is None:
        return next(g for g in (16, 8, 4, 2, 1) if tile % g == 0)
    cell = int(cell)
    if not 1 <= cell <= 64:
        raise ValueError("importance crops: cell=%d (1 .. 64)" % cell)
    if tile % cell != 0:
        raise ValueError("importance crops: cell=%d does not divide the tile of %d pixels" % (cell, tile))
    return cell


def cell_table(bank, G):
    """The dd_importance_cell table of a bank: the cells (cy, cx), cy < h // G, cx < w // G, row-major, scenes in order."""
    parts = []
    for s, scene in enumerate(bank.scenes):
        hc, wc = scene.height // G, scene.width // G
        t = np.zeros((hc, wc), dtype=CELL_DTYPE)
        t["source_plane0"], t["target_plane"] = bank.source_plane(s, 0), bank.target_plane(s)
        t["y0"], t["x0"] = (np.arange(hc, dtype=np.int32) * G)[:, None], (np.arange(wc, dtype=np.int32) * G)[None, :]
        parts.append(t.reshape(-1))
    return np.concatenate(parts)


class ImportanceMap:
    """The density of a bank's lattice windows and the draw from it (module docstring).  cells[s]: float64 [h // G, w // G], the mean SMAPE of
    the cells of scene s; weights[s]: float64 [(h - T) // G + 1, (w - T) // G + 1], the lattice windows' weights."""

    def __init__(self, bank, cell=None, floor=DEFAULT_FLOOR):
        import torch
        from . import _lib as L
        passes, G = colour_passes(bank), resolve_cell(bank.tile, cell)
        if len(passes) > L.IMPORTANCE_MAX_PASSES:
            raise ValueError("importance crops: %d colour passes, %d fit one launch" % (len(passes), L.IMPORTANCE_MAX_PASSES))
        table = cell_table(bank, G)
        desc = L.ImportanceDesc()
        desc.n_passes, desc.n_planes, desc.plane_hw, desc.n_sources, desc.epsilon = len(passes), bank.n_planes, bank.plane_hw.data_ptr(), bank.S, EPSILON
        for en, name in zip(desc.pass_, passes):
            en.planes = bank.pointers[name].data_ptr()
        with torch.cuda.device(bank.device):
            table_dev = torch.from_numpy(table.view(np.uint8).copy()).to(bank.device)
            out = torch.empty(len(table), dtype=torch.float64, device=bank.device)
            L.check(L.load().dd_importance_cells(C.byref(desc), table_dev.data_ptr(), len(table), G, out.data_ptr(),
                                                 torch.cuda.current_stream().cuda_stream))
            sums = out.cpu().numpy()                           # (one copy of the doubles; it waits for the launch)
        cells, at = [], 0
        for s, scene in enumerate(bank.scenes):
            hc, wc = scene.height // G, scene.width // G
            target = bank.target_plane(s)
            pairs = sum(1 for name in passes for k in range(bank.S)
                        if bank.planes[name][bank.source_plane(s, k)] is not None and bank.planes[name][target] is not None)
            block = sums[at:at + hc * wc].reshape(hc, wc)
            cells.append(block / (G * G * 3 * pairs) if pairs else np.zeros((hc, wc)))
            at += hc * wc
        self._finish(bank, cells, G, floor, passes)

    @classmethod
    def from_cells(cls, bank_like, cells, cell=None, floor=DEFAULT_FLOOR):
        """The same object from given cell means, without a device or the library.  bank_like: `.tile` and `.scenes` (each with `.height` and
        `.width`); cells: per scene an array [h // G, w // G]."""
        self = cls.__new__(cls)
        self._finish(bank_like, [np.asarray(c, dtype=np.float64) for c in cells], resolve_cell(bank_like.tile, cell), floor, None)
        return self

    def _finish(self, bank, cells, G, floor, passes):
        floor = float(floor)
        if not 0.0 <= floor <= 1.0:                            # (a NaN fails both comparisons)
            raise ValueError("importance crops: floor=%r (0 .. 1)" % (floor,))
        self.tile, self.cell, self.floor, self.passes = int(bank.tile), G, floor, passes
        self.sizes = [(s.height, s.width) for s in bank.scenes]
        if len(cells) != len(self.sizes):
            raise ValueError("importance crops: %d cell arrays for %d scenes" % (len(cells), len(self.sizes)))
        T, m = self.tile, self.tile // G
        self.cells, self.weights = [], []
        for (h, w), c in zip(self.sizes, cells):
            if c.shape != (h // G, w // G):
                raise ValueError("importance crops: cells of shape %s for a scene of %d x %d and cells of %d" % (c.shape, h, w, G))
            integral = np.zeros((c.shape[0] + 1, c.shape[1] + 1), dtype=np.float64)
            integral[1:, 1:] = c.cumsum(axis=0).cumsum(axis=1)
            ni, nj = (h - T) // G + 1, (w - T) // G + 1
            W = integral[m:m + ni, m:m + nj] - integral[:ni, m:m + nj] - integral[m:m + ni, :nj] + integral[:ni, :nj]
            self.cells.append(c)
            self.weights.append(np.maximum(W, 0.0))            # (the four-corner difference of a region of zeros may leave -1 ulp)
        self.n_lattice = [W.size for W in self.weights]
        self.offsets = np.concatenate([[0], np.cumsum(self.n_lattice)]).astype(np.int64)
        self.total = float(sum(W.sum() for W in self.weights))
        self.cdf = np.cumsum(np.concatenate([p.reshape(-1) for p in self.probabilities()]), dtype=np.float64)

    def fold(self, sums, counts, rate):
        """Move the visited cells towards the model's error there (ImportanceScorer.collect): for every cell with counts > 0,
        m = sums / 2^32 / counts and cells = (1 - rate) cells + rate m in float64; every other cell keeps its bytes.  sums, counts: flat integer
        tables over all cells, scenes in order, row-major (cell_table's order).  Weights, total, cdf and n_lattice are rebuilt by _finish; the
        draw contract is untouched.  Returns the number of cells folded."""
        from types import SimpleNamespace
        rate = float(rate)
        if not 0.0 < rate <= 1.0:                              # (a NaN fails both comparisons)
            raise ValueError("importance crops: rate=%r (above 0, at most 1)" % (rate,))
        sums, counts = np.asarray(sums).reshape(-1), np.asarray(counts).reshape(-1)
        n = sum(c.size for c in self.cells)
        if sums.shape != (n,) or counts.shape != (n,):
            raise ValueError("importance crops: tables of %d sums and %d counts for %d cells" % (sums.size, counts.size, n))
        cells, at, folded = [], 0, 0
        for c in self.cells:
            cnt = counts[at:at + c.size].reshape(c.shape)
            visited = cnt > 0
            new = c.copy()
            m = sums[at:at + c.size].reshape(c.shape)[visited].astype(np.float64) / 4294967296.0 / cnt[visited].astype(np.float64)
            new[visited] = (1.0 - rate) * c[visited] + rate * m
            cells.append(new)
            folded += int(visited.sum())
            at += c.size
        like = SimpleNamespace(tile=self.tile, scenes=[SimpleNamespace(height=h, width=w) for h, w in self.sizes])
        self._finish(like, cells, self.cell, self.floor, self.passes)
        return folded

    def probabilities(self):
        """Per scene the float64 array of the lattice windows' probabilities; they sum to 1 over all scenes."""
        n = len(self.weights)
        uniform = [np.full(W.shape, 1.0 / (n * W.size), dtype=np.float64) for W in self.weights]
        if self.total == 0.0:
            return uniform
        return [(1.0 - self.floor) * (W / self.total) + self.floor * U for W, U in zip(self.weights, uniform)]

    def draw(self, rng, index_tuples):
        """One example: (scene, y0, x0, index tuple), by the documented order of calls on `rng`."""
        x = rng.random() * self.cdf[-1]
        k = min(int(np.searchsorted(self.cdf, x, side="right")), len(self.cdf) - 1)      # the first index with cdf > x
        s = int(np.searchsorted(self.offsets, k, side="right")) - 1
        (h, w), G, T = self.sizes[s], self.cell, self.tile
        i, j = divmod(k - int(self.offsets[s]), self.weights[s].shape[1])
        y0 = min(i * G + rng.randrange(G), h - T)
        x0 = min(j * G + rng.randrange(G), w - T)
        return s, y0, x0, index_tuples[rng.randrange(len(index_tuples))]

    def heaviest_tenth_share(self):
        """The share of the total weight the heaviest tenth of the lattice windows holds (0 when there is no weight)."""
        if self.total == 0.0:
            return 0.0
        flat = np.sort(np.concatenate([W.reshape(-1) for W in self.weights]))[::-1]
        return float(flat[:-(-len(flat) // 10)].sum() / flat.sum())

    def describe(self):
        """The line rank 0 prints."""
        return ("frames: importance crops -- cells of %d, %d lattice windows, passes %s, floor %g, the heaviest tenth of the windows holds %.1f %% "
                "of the weight" % (self.cell, int(self.offsets[-1]), ", ".join(self.passes) if self.passes else "(given cells)", self.floor,
                                   100.0 * self.heaviest_tenth_share()))

    def picture(self, s):
        """The lattice weights of scene s as an 8-bit gray image [(h - T) // G + 1, (w - T) // G + 1], scaled by the set's largest weight
        (summaries.encode_png)."""
        top = max(float(W.max()) for W in self.weights)
        if top == 0.0:
            return np.zeros(self.weights[s].shape, dtype=np.uint8)
        return np.rint(255.0 * self.weights[s] / top).astype(np.uint8)


def cell_bases(bank, G):
    """(cell_base, n_cells) of a bank: int32 per plane, for a target plane the index of its scene's first cell in cell_table's order, -1 for
    every other plane."""
    base, at = np.full(bank.n_planes, -1, dtype=np.int32), 0
    for s, scene in enumerate(bank.scenes):
        base[bank.target_plane(s)] = at
        at += (scene.height // G) * (scene.width // G)
    return base, at


def reduce_tables(sums, counts, dist, device=None, group=None):
    """The tables of all ranks added: ONE all_reduce(SUM) of int64 over [sums | counts] -- integers, so the result is exact and the same
    bytes on every rank.  device: where the collective's tensor lives (the GPU under RCCL, None: the host, gloo)."""
    import torch
    n = len(sums)
    packed = torch.from_numpy(np.concatenate([np.asarray(sums, dtype=np.uint64).view(np.int64), np.asarray(counts).astype(np.int64)]))
    if device is not None:
        packed = packed.to(device)
    dist.all_reduce(packed, op=dist.ReduceOp.SUM, group=group)
    packed = packed.cpu().numpy()
    return packed[:n].view(np.uint64).copy(), packed[n:].astype(np.uint32)


class ImportanceScorer:
    """Scores every training step's mini-batch by the model's error (module docstring): one dd_importance_update launch in
    `program.step_tail_ops`, over the head features that are loaded, have 3 channels and are named in `importance.passes`, at scale 0.
    acc_sum (uint64) / acc_count (uint32): the flat device tables over all cells (torch holds them as int64 / int32: the same bytes)."""

    def __init__(self, program, sampler, importance):
        import torch
        from . import _lib as L
        from .loss_desc import block_ptr
        bank, B, T, G = sampler.bank, program.B, importance.tile, importance.cell
        if program.H != T or program.W != T or sampler.importance is not importance:
            raise ValueError("importance refresh: the map is not the one attached to this sampler, or the program was built for other tiles")
        wanted = list(importance.passes or ())
        index = {f.name: i for i, f in enumerate(program.head) if f.load_data and f.number_of_channels == 3}
        self.passes = [name for name in wanted if name in index]      # (the map's order: with the source in place of the prediction, its sums)
        if not self.passes:
            raise ValueError("importance refresh: the network predicts none of the colour passes the map was scored on (%s)" % ", ".join(wanted))
        self.program, self.sampler, self.importance, self.B, self.T, self.G = program, sampler, importance, B, T, G
        P, targets = program.predictions[0], program.targets[0]
        assert P.dtype == "f32" and targets.dtype == torch.float32
        d = self.desc = L.ImportanceUpdateDesc()
        d.n_passes, d.n_planes, d.plane_hw, d.epsilon = len(self.passes), bank.n_planes, bank.plane_hw.data_ptr(), EPSILON
        for en, name in zip(d.pass_, self.passes):
            i = index[name]
            en.pred, en.pred_ld = block_ptr(P, i * B), P.ld
            en.target, en.target_ld = targets.data_ptr() + i * B * T * T * int(targets.shape[-1]) * 4, int(targets.shape[-1])
        base, self.n_cells = cell_bases(bank, G)
        self.device = bank.device
        self.cell_base = torch.from_numpy(base).to(bank.device)
        d.cell_base = self.cell_base.data_ptr()
        self.acc_sum = torch.zeros(self.n_cells, dtype=torch.int64, device=bank.device)
        self.acc_count = torch.zeros(self.n_cells, dtype=torch.int32, device=bank.device)
        # training always samples with draws, so the switches dd_sample_tiles was given are constants of the sampler's usage
        flip, rotate = int(bool(sampler.usage.use_flip_left_right)), int(bool(sampler.usage.use_rotate_90))
        lib, records = L.load(), sampler._records_dev

        def run(stream, d=d, keep=(P.buf, targets, records, self.cell_base, self.acc_sum, self.acc_count)):
            L.check(lib.dd_importance_update(C.byref(d), records.data_ptr(), B, T, G, flip, rotate, self.acc_sum.data_ptr(),
                                             self.acc_count.data_ptr(), stream))
        run.info = None
        self.op = run
        program.add_step_tail_op(run, "importance_update")

    def tables(self):
        """(sums uint64, counts uint32) as they stand on the device (waits for the stream)."""
        return self.acc_sum.cpu().numpy().view(np.uint64), self.acc_count.cpu().numpy().view(np.uint32)

    def collect(self, dist=None):
        """(sums, counts) since the last call, added over the ranks of `dist` (torch.distributed, every rank calls); the device tables are
        zeroed.  Copying them to the host waits for the stream."""
        sums, counts = self.tables()
        self.acc_sum.zero_()
        self.acc_count.zero_()
        if dist is not None:
            sums, counts = reduce_tables(sums, counts, dist, device=self.device)
        return sums, counts
