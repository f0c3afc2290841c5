"""k_mock_draw at the edges of its 256-stored-pixel tile and its order-preserving count
(tests/model_spectra_edge_cases.py: MOCK_CASES) against the NumPy-and-oracle restatement
(tests/mock_restatement.py): 255, 256 and 257 stored pixels, no pixel outside the range, a first and a last
tile wholly outside it (the count of grid pixels before a tile stays 0 after a whole tile), the range
starting on a tile edge with a masked pixel, the in-range edges inside tile 0 and tile 1, a one-pixel
spectrum; with and without a mask and an absorber, at k = 20 and k = 40.  The tolerances are those of
tests/test_gpu_mocks.py (its _parity); every figure is printed before it is asserted."""
import numpy as np
import pytest

import gp_dla_detection_amd as gp

import mock_restatement as MR
import model_spectra_edge_cases as E
from test_gpu_mocks import SEED, TOL_DRAW, TOL_MAP, TOL_NORMAL, _context, _parity, _sizes, _upload

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("k", E.MOCK_RANKS)
def test_draw_at_the_tile_edges(oracle, k):
    c = E.mock_case(oracle, k)
    T = c["templates"]
    ctx = _context(c["model"], c["samples"])
    batch = _upload(ctx, T)
    try:
        res = batch.draw_mocks(c["truth"], seed=SEED, write_resident=False, components=("absorption", "continuum", "sigma", "latents"))
        counts = batch.unmasked_counts()
    finally:
        batch.close()
        ctx.close()
    np.testing.assert_array_equal(counts, [n for n, _, _ in E.MOCK_CASES])
    np.testing.assert_array_equal(np.diff(res["grid_offsets"]), counts)
    assert res["status"].tolist() == [0] * len(T) and res["latents"].shape == (len(T), k) and np.isfinite(res["latents"]).all()
    o = _sizes(T)
    assert res["flux"].size == o[-1] == sum(n + 2 * e for n, e, _ in E.MOCK_CASES)
    cells = {name: gp.split_cells(res[name], res["grid_offsets"]) for name in ("absorption", "continuum", "sigma")}
    outside = masked_inside = 0
    for i, (sp, (n, edge, mask)) in enumerate(zip(T, E.MOCK_CASES)):
        got = res["flux"][o[i]:o[i + 1]]
        inside, masked = E.in_range(sp), np.asarray(sp["pixel_mask"]) != 0
        assert inside.sum() == n and inside.size == n + 2 * edge
        # stored pixels outside the range keep their uploaded flux, bit for bit
        assert np.array_equal(got[~inside].view(np.uint64), np.asarray(sp["flux"], dtype=np.float64)[~inside].view(np.uint64)), (n, edge)
        outside += int((~inside).sum())
        # masked in-range pixels are NaN in flux, continuum and sigma; kept ones are numbers
        assert np.isnan(got[inside & masked]).all() and np.isfinite(got[inside & ~masked]).all(), (n, edge)
        for name in ("continuum", "sigma"):
            assert np.array_equal(np.isnan(cells[name][i]), masked[inside]), (n, edge, name)
        assert np.isfinite(cells["absorption"][i]).all() and cells["absorption"][i].size == n
        masked_inside += int((inside & masked).sum())
        if mask == "first":
            assert masked[inside][0] and np.isnan(got[edge]) and np.isfinite(got[edge + 1])
        want = MR.draw(oracle, c["model"], sp, i, SEED, *MR.absorbers_of(c["truth"], i))
        assert want["status"] == 0 and np.isfinite(want["flux"][inside & ~masked]).all() and np.isfinite(want["absorption"]).all()
    assert outside == sum(2 * e for _, e, _ in E.MOCK_CASES) > 1000 and masked_inside >= 4
    worst = _parity(oracle, c, res, meanflux=False)
    print(f"k = {k}, draw at the tile edges, worst |delta|:", {name: f"{v:.2e}" for name, v in worst.items()})
    assert np.abs(res["latents"]).max() <= 8.58
    assert worst["latents"] < TOL_NORMAL
    assert worst["absorption"] < TOL_MAP
    assert max(worst["flux"], worst["continuum"], worst["sigma"]) < TOL_DRAW
