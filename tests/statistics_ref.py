"""The reference's data-set statistics restated in numpy float64 (TEST INFRASTRUCTURE ONLY): TFRecordsStatistics.compute_and_save_statistics
as a true TWO-sweep over a list of tiles -- the first sweep for minimum, maximum, mean and coverage (:109-159, _first_statistics_iteration
:236-285), the second for the variance about the joined mean (:162-205, _second_statistics_iteration :287-316).  No shifted sums: this is what
the one-read reduction of deepdenoiser_amd/statistics.py is compared with.

A tile is (source_features, target_features): {Naming.source_feature_name(pass, samples_per_pixel=spp, index=i): [T, T, C]} and
{Naming.target_feature_name(pass): [T, T, C]}.  `target_from_last_source=True` reproduces the reference's slip (:132, :185): the unmasked
target entries are computed from the LAST source feature of the loops instead of the target feature.
"""
import numpy as np

from deepdenoiser_amd.naming import Naming
from deepdenoiser_amd.render_passes import RenderPasses


def signed_log1p(x):
    return np.sign(x) * np.log1p(np.abs(x))


def non_zero_mask(x):
    return np.sign(np.abs(x).sum(axis=2))


def has_masked_entry(render_pass):
    return RenderPasses.is_direct_or_indirect_render_pass(render_pass) and not RenderPasses.is_volume_render_pass(render_pass)


def _visits(tile, source_passes, target_passes, spps, sources, target_from_last_source):
    """The (feature, pass name, entry name, use_mask) calls the reference makes for one tile, in its order."""
    source_features, target_features = tile
    source_feature = None
    for spp in spps:
        for index in range(sources):
            for name in source_passes:
                source_feature = np.asarray(source_features[Naming.source_feature_name(name, samples_per_pixel=spp, index=index)], dtype=np.float64)
                yield source_feature, name, Naming.source_feature_name(name), False
                if has_masked_entry(name):
                    yield source_feature, name, Naming.source_feature_name(name, masked=True), True
    for name in target_passes:
        target_feature = np.asarray(target_features[Naming.target_feature_name(name)], dtype=np.float64)
        yield (source_feature if target_from_last_source else target_feature), name, Naming.target_feature_name(name), False
        if has_masked_entry(name):
            yield target_feature, name, Naming.target_feature_name(name, masked=True), True


def _mask(tile, render_pass):
    color = RenderPasses.direct_or_indirect_to_color_render_pass(render_pass)
    mask = non_zero_mask(np.asarray(tile[1][Naming.target_feature_name(color)], dtype=np.float64))
    return np.stack([mask, mask, mask], axis=2), mask.sum()


def statistics_ref(tiles, source_passes, target_passes, spps, sources, target_from_last_source=False):
    """{entry name: {"number_of_channels", "statistics": {...}, "statistics_log1p": {...}}} over `tiles` and the counts `spps`."""
    names = []
    for passes, feature_name in ((source_passes, Naming.source_feature_name), (target_passes, Naming.target_feature_name)):
        for p in passes:
            names.append(feature_name(p))
            if has_masked_entry(p):
                names.append(feature_name(p, masked=True))
    acc = {n: {"min": np.inf, "max": -np.inf, "minl": np.inf, "maxl": -np.inf, "means": [], "meansl": [], "coverage": [], "vars": [], "varsl": []}
           for n in names}
    # ---- first sweep
    for tile in tiles:
        for feature, render_pass, name, use_mask in _visits(tile, source_passes, target_passes, spps, sources, target_from_last_source):
            a, log = acc[name], signed_log1p(feature)
            a["min"], a["max"] = min(a["min"], feature.min()), max(a["max"], feature.max())
            a["minl"], a["maxl"] = min(a["minl"], log.min()), max(a["maxl"], log.max())
            cover = non_zero_mask(feature - 1.0 if RenderPasses.ALPHA in name else feature)
            if use_mask:
                mask, mask_sum = _mask(tile, render_pass)
                if mask_sum > 0:
                    a["means"].append((feature * mask / mask_sum).sum())
                    a["coverage"].append((cover / mask_sum).sum())
                    a["meansl"].append((log * mask / mask_sum).sum())
            else:
                a["means"].append(feature.mean())
                a["coverage"].append(cover.mean())
                a["meansl"].append(log.mean())
    joined = {n: {k: (float(np.mean(a[k])) if a[k] else 0.0) for k in ("means", "meansl", "coverage")} for n, a in acc.items()}
    # ---- second sweep
    for tile in tiles:
        for feature, render_pass, name, use_mask in _visits(tile, source_passes, target_passes, spps, sources, target_from_last_source):
            a, log = acc[name], signed_log1p(feature)
            mean, meanl = joined[name]["means"], joined[name]["meansl"]
            if use_mask:
                mask, mask_sum = _mask(tile, render_pass)
                if mask_sum > 0:
                    a["vars"].append((np.square(feature - mean) * mask / mask_sum).sum())
                    a["varsl"].append((np.square(log - meanl) * mask / mask_sum).sum())
            else:
                a["vars"].append(np.square(feature - mean).mean())
                a["varsl"].append(np.square(log - meanl).mean())
    out = {}
    for n, a in acc.items():
        j = joined[n]
        var, varl = (float(np.mean(a[k])) if a[k] else 0.0 for k in ("vars", "varsl"))
        out[n] = {"number_of_channels": RenderPasses.number_of_channels(n.split("/")[-1]),
                  "statistics": {"minimum": float(a["min"]), "maximum": float(a["max"]), "mean": j["means"], "variance": var, "coverage": j["coverage"]},
                  "statistics_log1p": {"minimum": float(a["minl"]), "maximum": float(a["maxl"]), "mean": j["meansl"], "variance": varl,
                                       "coverage": j["coverage"]}}
    return out


def pass_image(rng, h, w, name):
    """A seeded [h, w, C] float32 image of a pass with the traits the statistics must cope with: radiance is not negative, Alpha holds exact
    1.0 and 0.0 samples, Depth holds Blender's 1e10 (no surface hit) in a part of the image."""
    ch = RenderPasses.number_of_channels(name)
    img = rng.standard_normal((h, w, ch)).astype(np.float32)
    if RenderPasses.is_rgb_color_render_pass(name) or name == "Alpha":
        img = np.abs(img)
    if name == "Alpha":
        img[rng.random((h, w)) < 0.4] = 1.0
        img[rng.random((h, w)) < 0.2] = 0.0
    elif name == "Depth":
        img = np.abs(img) + 1.0
        img[rng.random((h, w)) < 0.3] = 1e10
    elif RenderPasses.is_rgb_color_render_pass(name):
        img[rng.random((h, w)) < 0.1] = 0.0          # black pixels: coverage below 1
    return img


def make_tiles(case):
    """The seeded tiles of a case of tests/golden/statistics_golden.json: {"seed", "tile", "tiles", "sources", "spps", "source_passes",
    "target_passes", "black_tile", "partly_black_tile"}.  In the black tile every target pass a mask is taken from is zero everywhere, in
    the partly black one in its upper half."""
    rng = np.random.default_rng(case["seed"])
    T = case["tile"]
    colors = {RenderPasses.direct_or_indirect_to_color_render_pass(p) for p in case["source_passes"] + case["target_passes"] if has_masked_entry(p)}
    tiles = []
    for n in range(case["tiles"]):
        source = {Naming.source_feature_name(p, samples_per_pixel=spp, index=i): pass_image(rng, T, T, p)
                  for spp in case["spps"] for i in range(case["sources"]) for p in case["source_passes"]}
        target = {Naming.target_feature_name(p): pass_image(rng, T, T, p) for p in case["target_passes"]}
        for p in colors:
            if n == case["black_tile"]:
                target[Naming.target_feature_name(p)][...] = 0.0
            elif n == case["partly_black_tile"]:
                target[Naming.target_feature_name(p)][:T // 2] = 0.0
        tiles.append((source, target))
    return tiles


def rows_ref(window, mask_window, is_alpha, field_names):
    """One row of dd_tile_statistics in numpy float64 for the window [T, T, C] of a pass (None: the pass is absent) and the window [T, T, 3]
    of its mask pass (None: no mask), in the header's field order."""
    row = dict.fromkeys(field_names, 0.0)
    if window is not None:
        x = np.asarray(window, dtype=np.float64)
        log = signed_log1p(x)
        K = x.reshape(-1)[0]
        Kl = float(signed_log1p(K))
        row.update(present=1.0, min=x.min(), max=x.max(), min_log1p=log.min(), max_log1p=log.max(), pivot=K, pivot_log1p=Kl,
                   sum=(x - K).sum(), sum_sq=np.square(x - K).sum(), sum_log1p=(log - Kl).sum(), sum_sq_log1p=np.square(log - Kl).sum(),
                   count=non_zero_mask(x - 1.0 if is_alpha else x).sum())
        if mask_window is not None:
            m = non_zero_mask(np.asarray(mask_window, dtype=np.float64))
            m3 = m[:, :, None]
            row.update(mask_sum=m.sum(), masked_sum=((x - K) * m3).sum(), masked_sum_sq=(np.square(x - K) * m3).sum(),
                       masked_sum_log1p=((log - Kl) * m3).sum(), masked_sum_sq_log1p=(np.square(log - Kl) * m3).sum())
    return np.array([row[k] for k in field_names], dtype=np.float64)


def entries_differ(a, b, rtol):
    """The keys whose entries differ by more than `rtol` (relative, per number; both 0 or both infinite of one sign count as equal)."""
    bad = []
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b or a[name]["number_of_channels"] != b[name]["number_of_channels"]:
            bad.append(name)
            continue
        for section in ("statistics", "statistics_log1p"):
            for key in ("minimum", "maximum", "mean", "variance", "coverage"):
                u, v = a[name][section][key], b[name][section][key]
                if not (u == v or abs(u - v) <= rtol * max(abs(u), abs(v))):
                    bad.append(name)
    return sorted(set(bad))
