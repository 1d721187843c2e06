"""tests/statistics_ref.py against the reference itself: tests/golden/statistics_golden.json holds what TFRecordsStatistics.py wrote for seeded
tiles (tests/golden/make_statistics_golden.py ran the reference's module on a float64 stand-in for TensorFlow).  Both sides are float64 and
follow the same rules; only the order of the sums differs (torch's reductions there, numpy's here), hence rtol 1e-12: a few hundred summands
of one sign or of moderate cancellation each carry at most n * 2^-53 ~ 1e-13."""
import json
import os

import pytest

import statistics_ref as R
from deepdenoiser_amd.naming import Naming

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "statistics_golden.json")) as f:
    GOLDEN = json.load(f)
CASES = {c["name"]: c for c in GOLDEN["cases"]}
KEYS = [(name, key) for name, c in sorted(CASES.items()) for key in sorted(c["results"])]
_TILES = {}


def tiles_of(case):
    if case["name"] not in _TILES:
        _TILES[case["name"]] = R.make_tiles(case)
    return _TILES[case["name"]]


def run(case, key, slip):
    spps = case["spps"] if key == "all" else [int(key)]
    return R.statistics_ref(tiles_of(case), case["source_passes"], case["target_passes"], spps, case["sources"], target_from_last_source=slip)


def test_golden_covers_the_cases_the_statistics_must_cope_with():
    assert {c["group"] for c in CASES.values()} == {False, True}
    for c in CASES.values():
        assert c["sources"] == 2 and len(c["spps"]) == 2
        assert {"Diffuse Color", "Diffuse Direct", "Glossy Indirect", "Volume Direct", "Alpha", "Depth", "Normal"} <= set(c["source_passes"])
        assert c["black_tile"] != c["partly_black_tile"] and max(c["black_tile"], c["partly_black_tile"]) < c["tiles"]
        assert sorted(c["results"]) == (sorted(str(s) for s in c["spps"]) if c["group"] else ["all"])


@pytest.mark.parametrize("name,key", KEYS)
def test_reference_with_the_slip_equals_the_golden(name, key):
    case = CASES[name]
    have, want = run(case, key, True), case["results"][key]
    assert sorted(have) == sorted(want)
    assert R.entries_differ(have, want, 1e-12) == []
    # masked entries exist exactly for the direct / indirect passes that are no volume passes
    masked = sorted(n for n in have if n.endswith(" Masked"))
    assert masked == sorted([Naming.source_feature_name(p, masked=True) for p in ("Diffuse Direct", "Glossy Indirect")]
                            + [Naming.target_feature_name(p, masked=True) for p in ("Diffuse Direct", "Glossy Indirect")])


@pytest.mark.parametrize("name,key", KEYS)
def test_without_the_slip_exactly_the_unmasked_target_entries_differ(name, key):
    case = CASES[name]
    have, want = run(case, key, False), case["results"][key]
    assert R.entries_differ(have, want, 1e-12) == sorted(Naming.target_feature_name(p) for p in case["target_passes"])
