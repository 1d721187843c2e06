"""Generates tests/golden/statistics_golden.json by EXECUTING the reference's TFRecordsStatistics.compute_and_save_statistics
(TFRecordsStatistics.py:26-233) on seeded tiles.

The reference's module is IMPORTED from /root/reference at generation time on a small float64 stand-in for the `tf` names it and
Utilities.py / Conv2dUtilities.py use (this file's own: torch float64 tensors, which have the `.numpy().item()` the reference calls).
`_dataset_iterator` (:318-367, the tile set on disk) is replaced by an iterator over the tiles of tests/statistics_ref.make_tiles, and
`tfrecords_creator` by a plain object with the attributes the class reads.  The arithmetic is float64 where TensorFlow's is float32: the
fixture pins the reference's RULES (which windows, which divisor, which mask, the :132 / :185 slip), not TensorFlow's rounding.

Nothing of the reference travels: the JSON holds the cases (seeds, shapes, pass names) and the statistics it wrote.  Run in the build
container only:
    python tests/golden/make_statistics_golden.py
"""
import json
import os
import sys
import tempfile
import types

import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
REF = "/root/reference/TensorFlow"

SOURCE_PASSES = ["Alpha", "Depth", "Normal", "Diffuse Color", "Diffuse Direct", "Glossy Indirect", "Volume Direct"]
TARGET_PASSES = ["Alpha", "Depth", "Diffuse Color", "Diffuse Direct", "Glossy Indirect", "Volume Direct"]
CASES = [
    {"name": "ungrouped", "group": False, "seed": 41, "tile": 6, "tiles": 5, "sources": 2, "spps": [4, 16],
     "source_passes": SOURCE_PASSES, "target_passes": TARGET_PASSES, "black_tile": 1, "partly_black_tile": 3},
    {"name": "grouped", "group": True, "seed": 42, "tile": 5, "tiles": 4, "sources": 2, "spps": [4, 16],
     "source_passes": SOURCE_PASSES, "target_passes": TARGET_PASSES, "black_tile": 0, "partly_black_tile": 2},
]


class OutOfRangeError(Exception):
    pass


def _t(x):
    if isinstance(x, torch.Tensor):
        return x
    if isinstance(x, (list, tuple)):
        return torch.stack([_t(v) for v in x])
    return torch.as_tensor(x, dtype=torch.float64)


def _reduce(f):
    return lambda x, axis=None: f(_t(x)) if axis is None else f(_t(x), dim=axis)


def tf_stand_in():
    tf = types.ModuleType("tensorflow")
    for name, f in (("minimum", torch.minimum), ("maximum", torch.maximum), ("multiply", torch.mul), ("divide", torch.div),
                    ("subtract", torch.sub), ("greater", torch.gt)):
        setattr(tf, name, (lambda f: lambda a, b: f(_t(a), _t(b)))(f))
    for name, f in (("abs", torch.abs), ("sign", torch.sign), ("square", torch.square), ("log1p", torch.log1p), ("expm1", torch.expm1)):
        setattr(tf, name, (lambda f: lambda a: f(_t(a)))(f))
    tf.reduce_sum, tf.reduce_mean = _reduce(torch.sum), _reduce(torch.mean)
    tf.reduce_min, tf.reduce_max = _reduce(torch.amin), _reduce(torch.amax)
    tf.stack = lambda values, axis=0: torch.stack([_t(v) for v in values], dim=axis)
    tf.errors = types.SimpleNamespace(OutOfRangeError=OutOfRangeError)
    contrib = types.ModuleType("tensorflow.contrib")
    eager = types.ModuleType("tensorflow.contrib.eager")
    tf.contrib, contrib.eager = contrib, eager
    sys.modules.update({"tensorflow": tf, "tensorflow.contrib": contrib, "tensorflow.contrib.eager": eager})
    return tf


class TileIterator:
    def __init__(self, tiles):
        self.tiles = iter(tiles)

    def get_next(self):
        try:
            source, target = next(self.tiles)
        except StopIteration:
            raise OutOfRangeError()
        return ({k: torch.from_numpy(v).double() for k, v in source.items()}, {k: torch.from_numpy(v).double() for k, v in target.items()})


def run_case(RefStatistics, case, tiles, directory):
    """-> {"all" | str(spp): the statistics the reference wrote}"""
    creator = types.SimpleNamespace(
        group_by_samples_per_pixel=case["group"], source_samples_per_pixel_list=list(case["spps"]),
        number_of_sources_per_example=case["sources"], name=case["name"], base_tfrecords_directory=directory,
        tiles_height_width=case["tile"],
        source_render_passes_usage=types.SimpleNamespace(render_passes=lambda: list(case["source_passes"])),
        target_render_passes_usage=types.SimpleNamespace(render_passes=lambda: list(case["target_passes"])))
    statistics = RefStatistics(creator)
    statistics._dataset_iterator = lambda group, spps: TileIterator(tiles)
    statistics.compute_and_save_statistics()
    out = {}
    for key in ([str(s) for s in case["spps"]] if case["group"] else ["all"]):
        name = case["name"] + ("_statistics.json" if key == "all" else "_statistics_%s.json" % key)
        with open(os.path.join(directory, name), encoding="utf-8") as f:
            out[key] = json.load(f)
    return out


def main():
    tf_stand_in()
    sys.path.insert(0, REF)
    from TFRecordsStatistics import TFRecordsStatistics as RefStatistics      # (the reference's module, on the stand-in)
    import statistics_ref
    golden = {"cases": []}
    for case in CASES:
        tiles = statistics_ref.make_tiles(case)
        with tempfile.TemporaryDirectory() as directory:
            results = run_case(RefStatistics, case, tiles, directory)
        golden["cases"].append(dict(case, results=results))
        print("%-10s %d tiles of %d: %s" % (case["name"], case["tiles"], case["tile"],
                                             ", ".join("%s: %d entries" % (k, len(v)) for k, v in results.items())))
    path = os.path.join(HERE, "statistics_golden.json")
    with open(path, "w") as f:
        json.dump(golden, f, indent=1, sort_keys=True)
    assert os.path.getsize(path) < 1024 * 1024, os.path.getsize(path)
    print("wrote statistics_golden.json (%.1f KiB)" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
