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
is noise only: no structure term (target gradients, normals), no refresh from the running model's loss, and no loss re-weighting -- this is a
deliberate change of the training distribution, as in KPCN."""
import ctypes as C

import numpy as np

EPSILON = 1e-2            # LossDifference.difference's default epsilon
DEFAULT_FLOOR = 0.25      # a choice, not a measured optimum

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
