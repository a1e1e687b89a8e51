"""CPU: the one band-height search behind wm_lfss_in_conv_band_rows and wm_lfss_ffn_band_rows returns, for every size of the
recorded grid, what the two separate searches returned on the commit named in tests/golden/row_walk_band_rows.json (host
arithmetic only; tests/golden/make_golden_row_walk.py wrote the file)."""
import json
import os

import pytest

from wave_mamba_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "row_walk_band_rows.json")


@pytest.mark.parametrize("key", ["lfss_in_conv", "lfss_ffn"])
def test_band_rows_match_the_recorded_search(key):
    with open(GOLDEN) as f:
        g = json.load(f)
    sizes = [(B, H, W) for B in g["B"] for H in g["H"] for W in g["W"]]
    assert len(sizes) == len(g[key]) == 3 * 303 * 7
    fn = getattr(_lib.load(), f"wm_{key}_band_rows")
    wrong = [(s, want, fn(*s)) for s, want in zip(sizes, g[key]) if fn(*s) != want]
    assert not wrong, f"{len(wrong)} of {len(sizes)} sizes differ; first (size, recorded, now): {wrong[:5]}"
