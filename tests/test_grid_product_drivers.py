"""CPU checks of what the grid products -- model spectra, marginal continuum, predictive flux -- share above ``Batch``: the
field table (gp_dla_detection_amd/grid_fields.py), the one block loop of the drivers (``api.stitch_blocks``) over canned
blocks, the rule for the empty selection on every driver path, and the one saver body of ``io`` against files written by
the three separate savers it replaced (their contents recorded below as literals)."""
import numpy as np
import pytest

from gp_dla_detection_amd import api, grid_fields, hdf5, io, synthetic
from gp_dla_detection_amd.parameters import MultiParameters


# ------------------------------------------------------------------------------------------------
# the table behind the public tuples
# ------------------------------------------------------------------------------------------------

def test_public_tuples_keep_their_contents():
    assert api.MODEL_SPECTRA_ARRAYS == io.MODEL_SPECTRA_CELLS == ("map_absorption", "mean_absorption", "var_absorption", "continuum",
                                                                   "model_flux")
    assert api.MODEL_SPECTRA_MULTI_ARRAYS == io.MODEL_SPECTRA_MULTI_CELLS == ("mean_absorption_lls", "var_absorption_lls",
                                                                               "expected_absorption", "expected_var_absorption")
    assert api.MODEL_SPECTRA_MULTI_PLANES == io.MODEL_SPECTRA_MULTI_PLANE_CELLS == ("mean_absorption_models", "var_absorption_models")
    assert api.MARGINAL_CONTINUUM_ARRAYS == io.MARGINAL_CONTINUUM_CELLS == ("continuum_mean", "continuum_var", "continuum_var_between")
    assert api.MARGINAL_CONTINUUM_ROWS == ("coef_mean", "coef_cov_within", "coef_cov_between", "sample_coefficients")
    assert io.MARGINAL_CONTINUUM_MATRICES == ("coef_mean", "coef_cov_within", "coef_cov_between", "model_weights")
    assert api.PREDICTIVE_FLUX_ARRAYS == ("flux_mean", "flux_var", "flux_var_within", "flux_var_between", "noise_var")
    assert api.PREDICTIVE_FLUX_RESIDUALS == ("residual",)
    assert io.PREDICTIVE_FLUX_CELLS == api.PREDICTIVE_FLUX_ARRAYS + api.PREDICTIVE_FLUX_RESIDUALS
    assert api.PREDICTIVE_FLUX_ROWS == io.PREDICTIVE_FLUX_COLUMNS == ("chi2", "num_kept")


# ------------------------------------------------------------------------------------------------
# a. the block loop over canned blocks
# ------------------------------------------------------------------------------------------------

PIXELS = (5, 0, 33, 17, 64)     # the second quasar has no grid pixel
BLOCKS = (2, 2, 1)
MD, K = 3, 2


def _whole():
    """What the stitched result must be: every array of distinct entries, so that a misplaced block shows."""
    n, total = len(PIXELS), sum(PIXELS)
    return {"offsets": np.concatenate([[0], np.cumsum(PIXELS)]).astype(np.int64),
            "status": np.array([0, 1, 0, 4, 0], dtype=np.int32), "status_more": np.array([8, 0, 0, 8, 0], dtype=np.int32),
            "model_flags": np.array([1, 0, 2 ** 30, 3, 2 ** 31], dtype=np.uint32),
            "flux_mean": np.arange(total) + 0.5, "residual": -np.arange(total) - 0.25,
            "mean_absorption_models": np.arange(MD * total, dtype=np.float64).reshape(MD, total),
            "coef_mean": np.arange(n * K, dtype=np.float64).reshape(n, K),
            "sample_coefficients": np.arange(n * 4 * K, dtype=np.float64).reshape(n, 4, K),
            "chi2": np.arange(n) + 0.125, "num_kept": np.array([5, 0, 30, 17, 2 ** 40], dtype=np.int64)}


BY_NAME = {f.name: f for f in grid_fields.FIELDS}
# two pixel arrays and a plane (the first call of a block), two rows and two columns (a second call), the flags in front
EXPECT = tuple(BY_NAME[name] for name in ("model_flags", "flux_mean", "residual", "mean_absorption_models", "coef_mean",
                                          "sample_coefficients", "chi2", "num_kept"))


def _blocks(log):
    lo = 0
    for i, size in enumerate(BLOCKS):
        log.append(i)
        yield lo, lo + size, np.arange(lo, lo + size), f"batch {i}"
        lo += size


def _per_block(whole):
    def per_block(batch, idx, lo, hi):
        assert batch == f"batch {lo // 2}" and idx.tolist() == list(range(lo, hi))
        off = whole["offsets"]
        px = slice(off[lo], off[hi])
        first = {"offsets": off[lo:hi + 1] - off[lo], "status": whole["status"][lo:hi], "not_a_field": np.zeros(3)}
        for f in EXPECT[:4]:     # model_flags, flux_mean, residual, the plane: from the first call of the block
            first[f.name] = whole[f.name][..., px] if f.kind in ("pixel", "plane") else whole[f.name][lo:hi]
        second = {"offsets": first["offsets"], "status": whole["status_more"][lo:hi]}
        for f in EXPECT[4:]:     # the rows and the columns: from a second call
            second[f.name] = whole[f.name][lo:hi]
        return first, second
    return per_block


def test_blocks_are_stitched_in_selection_order():
    whole, log = _whole(), []
    got = api.stitch_blocks(_blocks(log), len(PIXELS), _per_block(whole), EXPECT, dict(k=K, samples=4, max_dlas=MD))
    assert log == [0, 1, 2]
    assert list(got) == ["offsets", "status", "model_flags", "flux_mean", "residual", "mean_absorption_models", "coef_mean",
                         "sample_coefficients", "chi2", "num_kept"]
    np.testing.assert_array_equal(got["status"], whole["status"] | whole["status_more"])      # the second call's status is OR-ed in
    assert got["status"].tolist() == [8, 1, 0, 12, 0] and got["status"].dtype == np.int32
    assert got["offsets"].dtype == np.int64 and got["offsets"].tolist() == [0, 5, 5, 38, 55, 119]
    for name in list(got)[2:]:
        assert got[name].dtype == whole[name].dtype and got[name].shape == whole[name].shape, name
        np.testing.assert_array_equal(got[name], whole[name], err_msg=name)
    assert got["model_flags"].dtype == np.uint32 and got["num_kept"].dtype == np.int64 and got["chi2"].dtype == np.float64
    assert got["mean_absorption_models"].shape == (MD, sum(PIXELS))


def test_one_dict_per_block_serves_and_a_missing_field_is_an_error():
    whole = _whole()
    per_block = _per_block(whole)
    expect = EXPECT[:4]
    got = api.stitch_blocks(_blocks([]), len(PIXELS), lambda *a: per_block(*a)[0], expect, dict(k=K, samples=4, max_dlas=MD))
    assert list(got) == ["offsets", "status", "model_flags", "flux_mean", "residual", "mean_absorption_models"]
    np.testing.assert_array_equal(got["status"], whole["status"])
    np.testing.assert_array_equal(got["flux_mean"], whole["flux_mean"])
    with pytest.raises(ValueError):     # a field the call should return and no block did: nothing to join
        api.stitch_blocks(_blocks([]), len(PIXELS), lambda *a: per_block(*a)[0], EXPECT, dict(k=K, samples=4, max_dlas=MD))


def test_no_block_is_asked_for_when_the_selection_is_empty():
    def never(*a):
        raise AssertionError("no block to call")
    got = api.stitch_blocks(iter(()), 0, never, EXPECT, dict(k=K, samples=4, max_dlas=MD), refined=dict(levels=3))
    assert list(got) == ["offsets", "status", "boxes", "refine_status"] + [f.name for f in EXPECT]
    assert got["boxes"].shape == (0, 3, 4) and got["refine_status"].dtype == np.int32
    assert got["mean_absorption_models"].shape == (MD, 0) and got["sample_coefficients"].shape == (0, 4, K)


# ------------------------------------------------------------------------------------------------
# b. the empty selection on every driver path
# ------------------------------------------------------------------------------------------------

F8, I8, I4, U4 = np.dtype(np.float64), np.dtype(np.int64), np.dtype(np.int32), np.dtype(np.uint32)
HEAD = [("selection", (0,), I8), ("offsets", (1,), I8), ("status", (0,), I4)]
FLAGS = [("model_flags", (0,), U4)]
REFINED = [("boxes", (0, 2, 4), F8), ("refine_status", (0,), I4)]
# as the parent returned them, with make_model(2), make_samples(4), sample_coefficients=True, residuals=True
MC = [(n, (0,), F8) for n in ("continuum_mean", "continuum_var", "continuum_var_between")] + [
    ("coef_mean", (0, 2), F8), ("coef_cov_within", (0, 3), F8), ("coef_cov_between", (0, 3), F8)]
PF = [(n, (0,), F8) for n in ("flux_mean", "flux_var", "flux_var_within", "flux_var_between", "noise_var", "residual", "chi2")] + [
    ("num_kept", (0,), I8)]
MS = [(n, (0,), F8) for n in ("map_absorption", "mean_absorption", "var_absorption", "continuum", "model_flux")]
MS_MULTI = [(n, (0,), F8) for n in ("mean_absorption_lls", "var_absorption_lls", "expected_absorption", "expected_var_absorption")] + [
    ("mean_absorption_models", (2, 0), F8), ("var_absorption_models", (2, 0), F8)]

EMPTY = {
    ("marginal_continuum", "plain"): HEAD + MC + [("sample_coefficients", (0, 4, 2), F8)],
    ("predictive_flux", "plain"): HEAD + PF,
    ("marginal_continuum", "multi_models"): HEAD + FLAGS + MC,
    ("predictive_flux", "multi_models"): HEAD + FLAGS + PF,
    # the rule of the one driver, where the parent returned ``selection``, ``offsets`` and ``status`` alone
    ("model_spectra", "plain"): HEAD + MS,
    ("model_spectra", "multi_models"): HEAD + FLAGS + MS + MS_MULTI,
    ("model_spectra", "refined"): HEAD + REFINED + MS,
    ("marginal_continuum", "refined"): HEAD + REFINED + MC + [("sample_coefficients", (0, 7, 2), F8)],     # S' = 7 points
    ("marginal_continuum", "refined_all_samples"): HEAD + REFINED + MC + [("sample_coefficients", (0, 4, 2), F8)],
    ("predictive_flux", "refined"): HEAD + REFINED + PF,
}


@pytest.mark.parametrize("product,path", list(EMPTY))
def test_empty_selection_returns_every_key(product, path, monkeypatch):
    model, samples = synthetic.make_model(2), synthetic.make_samples(4)
    spectra = synthetic.make_spectra(3, 40, model)
    monkeypatch.setattr(api, "_block_size", lambda *a: pytest.fail("an empty selection sizes no block"))
    kw = dict(selection=[])
    results = None
    if path == "multi_models":
        kw.update(params=MultiParameters(max_dlas=2), multi_models=True, model_weights=np.ones((3, 4)), multi_rows=lambda idx: {})
    elif path.startswith("refined"):
        results = dict(log_priors_no_dla=np.log(np.full(3, 0.9)), log_priors_dla=np.log(np.full(3, 0.1)))
        kw.update(refined=dict(levels=2, points=7) if path == "refined" else dict(levels=2))
    if product == "model_spectra":
        kw.update(absorbers=None, sample_rows=lambda idx: np.zeros((len(idx), 4)))
    elif product == "marginal_continuum":
        kw.update(sample_coefficients=path != "multi_models", sample_rows=lambda idx, name: np.zeros((len(idx), 4)))
    else:
        kw.update(residuals=True, sample_rows=lambda idx, name: np.zeros((len(idx), 4)))
    got = getattr(api, product)(model, samples, spectra, results, **kw)
    assert [(name, a.shape, a.dtype) for name, a in got.items()] == EMPTY[product, path]


# ------------------------------------------------------------------------------------------------
# c. the saver
# ------------------------------------------------------------------------------------------------

def _saver_inputs() -> dict:
    """One small result per saver: three quasars of 2, 0 and 3 grid pixels, refined on two levels, with ``model_flags``, and a
    plane or ``sample_coefficients`` where the saver takes them.  Keys in an order of their own: the file's is the saver's."""
    total = 5
    px = lambda a: a + np.arange(total) / 8.0      # noqa: E731
    head = {"model_flags": np.array([0, 2, 2 ** 30], dtype=np.uint32), "selection": np.array([4, 0, 7]),
            "offsets": np.array([0, 2, 2, 5]), "status": np.array([0, 1, 16], dtype=np.int32),
            "boxes": 2.0 + np.arange(24.0).reshape(3, 2, 4) / 16.0, "refine_status": np.array([0, -1, 3], dtype=np.int32)}
    ms = dict(head, var_absorption_models=np.arange(10.0).reshape(2, 5) / 4.0, mean_absorption_models=-np.arange(10.0).reshape(2, 5),
              expected_absorption=px(40.0), model_flux=px(10.0), map_absorption=px(20.0), mean_absorption_lls=px(30.0),
              absorber_offsets=np.array([0, 1, 1, 3]), absorber_z_dlas=np.array([2.5, 2.25, 3.0]),
              absorber_log_nhis=np.array([20.5, 21.0, 22.25]), not_a_product=np.zeros(3))
    mc = dict(head, sample_coefficients=np.arange(12.0).reshape(3, 2, 2), model_weights=np.arange(9.0).reshape(3, 3) / 8.0,
              coef_cov_between=np.arange(9.0).reshape(3, 3) + 0.5, coef_mean=np.arange(6.0).reshape(3, 2),
              coef_cov_within=-np.arange(9.0).reshape(3, 3), continuum_var=px(1.0), continuum_mean=px(2.0),
              continuum_var_between=px(3.0))
    pf = dict(head, num_kept=np.array([2, 0, 1], dtype=np.int64), chi2=np.array([1.5, 0.0, 0.25]), residual=px(-1.0), noise_var=px(5.0),
              flux_mean=px(6.0), flux_var=px(7.0), flux_var_within=px(8.0), flux_var_between=px(9.0),
              model_weights=np.arange(12.0).reshape(3, 4) / 4.0)
    return {"model_spectra": ms, "marginal_continuum": mc, "predictive_flux": pf}


def _plain(v):
    """A loaded variable as literals: (shape, nested lists) of an array, a list of those for a cell, a string as it is."""
    if isinstance(v, list):
        return [_plain(c) for c in v]
    if isinstance(v, str):
        return v
    a = np.asarray(v)
    return (a.shape, a.tolist())


def _saved(path: str) -> list:
    """``[(name, _plain(variable))]`` of a file in the order the variables were written: the writer appends, so that is the
    order of their object headers' addresses."""
    back = io.loadmat73(path)
    with hdf5.File(path) as f:
        order = sorted(back, key=lambda name: f[name].addr)
    return [(name, _plain(back[name])) for name in order]


# The files of the three separate savers of the parent commit for _saver_inputs() (metadata: processed_file="p.mat",
# multi_dla=np.float64(1)), as _saved() gives them.
SAVED = {'model_spectra': [('processed_file', 'p.mat'), ('multi_dla', ((1, 1), [[1.0]])), ('quasar_ind', ((3, 1), [[5.0], [1.0], [8.0]])),
                   ('num_pixels', ((3, 1), [[2.0], [0.0], [3.0]])), ('status', ((3, 1), [[0.0], [1.0], [16.0]])),
                   ('refine_boxes',
                    ((3, 8),
                     [[2.0, 2.0625, 2.125, 2.1875, 2.25, 2.3125, 2.375, 2.4375],
                      [2.5, 2.5625, 2.625, 2.6875, 2.75, 2.8125, 2.875, 2.9375],
                      [3.0, 3.0625, 3.125, 3.1875, 3.25, 3.3125, 3.375, 3.4375]])),
                   ('refine_status', ((3, 1), [[0.0], [-1.0], [3.0]])),
                   ('map_z_dlas', [((1, 1), [[2.5]]), ((0, 1), []), ((2, 1), [[2.25], [3.0]])]),
                   ('map_log_nhis', [((1, 1), [[20.5]]), ((0, 1), []), ((2, 1), [[21.0], [22.25]])]),
                   ('map_absorption', [((2, 1), [[20.0], [20.125]]), ((0, 1), []), ((3, 1), [[20.25], [20.375], [20.5]])]),
                   ('model_flux', [((2, 1), [[10.0], [10.125]]), ((0, 1), []), ((3, 1), [[10.25], [10.375], [10.5]])]),
                   ('mean_absorption_lls', [((2, 1), [[30.0], [30.125]]), ((0, 1), []), ((3, 1), [[30.25], [30.375], [30.5]])]),
                   ('expected_absorption', [((2, 1), [[40.0], [40.125]]), ((0, 1), []), ((3, 1), [[40.25], [40.375], [40.5]])]),
                   ('mean_absorption_models',
                    [((2, 2), [[-0.0, -5.0], [-1.0, -6.0]]), ((0, 2), []), ((3, 2), [[-2.0, -7.0], [-3.0, -8.0], [-4.0, -9.0]])]),
                   ('var_absorption_models',
                    [((2, 2), [[0.0, 1.25], [0.25, 1.5]]), ((0, 2), []), ((3, 2), [[0.5, 1.75], [0.75, 2.0], [1.0, 2.25]])]),
                   ('model_flags', ((3, 1), [[0.0], [2.0], [1073741824.0]]))],
 'marginal_continuum': [('processed_file', 'p.mat'), ('multi_dla', ((1, 1), [[1.0]])),
                        ('quasar_ind', ((3, 1), [[5.0], [1.0], [8.0]])), ('num_pixels', ((3, 1), [[2.0], [0.0], [3.0]])),
                        ('status', ((3, 1), [[0.0], [1.0], [16.0]])),
                        ('refine_boxes',
                         ((3, 8),
                          [[2.0, 2.0625, 2.125, 2.1875, 2.25, 2.3125, 2.375, 2.4375],
                           [2.5, 2.5625, 2.625, 2.6875, 2.75, 2.8125, 2.875, 2.9375],
                           [3.0, 3.0625, 3.125, 3.1875, 3.25, 3.3125, 3.375, 3.4375]])),
                        ('refine_status', ((3, 1), [[0.0], [-1.0], [3.0]])),
                        ('continuum_mean', [((2, 1), [[2.0], [2.125]]), ((0, 1), []), ((3, 1), [[2.25], [2.375], [2.5]])]),
                        ('continuum_var', [((2, 1), [[1.0], [1.125]]), ((0, 1), []), ((3, 1), [[1.25], [1.375], [1.5]])]),
                        ('continuum_var_between', [((2, 1), [[3.0], [3.125]]), ((0, 1), []), ((3, 1), [[3.25], [3.375], [3.5]])]),
                        ('coef_mean', ((3, 2), [[0.0, 1.0], [2.0, 3.0], [4.0, 5.0]])),
                        ('coef_cov_within', ((3, 3), [[-0.0, -1.0, -2.0], [-3.0, -4.0, -5.0], [-6.0, -7.0, -8.0]])),
                        ('coef_cov_between', ((3, 3), [[0.5, 1.5, 2.5], [3.5, 4.5, 5.5], [6.5, 7.5, 8.5]])),
                        ('model_weights', ((3, 3), [[0.0, 0.125, 0.25], [0.375, 0.5, 0.625], [0.75, 0.875, 1.0]])),
                        ('sample_coefficients',
                         [((2, 2), [[0.0, 1.0], [2.0, 3.0]]), ((2, 2), [[4.0, 5.0], [6.0, 7.0]]),
                          ((2, 2), [[8.0, 9.0], [10.0, 11.0]])]),
                        ('model_flags', ((3, 1), [[0.0], [2.0], [1073741824.0]]))],
 'predictive_flux': [('processed_file', 'p.mat'), ('multi_dla', ((1, 1), [[1.0]])),
                     ('quasar_ind', ((3, 1), [[5.0], [1.0], [8.0]])), ('num_pixels', ((3, 1), [[2.0], [0.0], [3.0]])),
                     ('status', ((3, 1), [[0.0], [1.0], [16.0]])),
                     ('refine_boxes',
                      ((3, 8),
                       [[2.0, 2.0625, 2.125, 2.1875, 2.25, 2.3125, 2.375, 2.4375],
                        [2.5, 2.5625, 2.625, 2.6875, 2.75, 2.8125, 2.875, 2.9375],
                        [3.0, 3.0625, 3.125, 3.1875, 3.25, 3.3125, 3.375, 3.4375]])),
                     ('refine_status', ((3, 1), [[0.0], [-1.0], [3.0]])),
                     ('flux_mean', [((2, 1), [[6.0], [6.125]]), ((0, 1), []), ((3, 1), [[6.25], [6.375], [6.5]])]),
                     ('flux_var', [((2, 1), [[7.0], [7.125]]), ((0, 1), []), ((3, 1), [[7.25], [7.375], [7.5]])]),
                     ('flux_var_within', [((2, 1), [[8.0], [8.125]]), ((0, 1), []), ((3, 1), [[8.25], [8.375], [8.5]])]),
                     ('flux_var_between', [((2, 1), [[9.0], [9.125]]), ((0, 1), []), ((3, 1), [[9.25], [9.375], [9.5]])]),
                     ('noise_var', [((2, 1), [[5.0], [5.125]]), ((0, 1), []), ((3, 1), [[5.25], [5.375], [5.5]])]),
                     ('residual', [((2, 1), [[-1.0], [-0.875]]), ((0, 1), []), ((3, 1), [[-0.75], [-0.625], [-0.5]])]),
                     ('chi2', ((3, 1), [[1.5], [0.0], [0.25]])), ('num_kept', ((3, 1), [[2.0], [0.0], [1.0]])),
                     ('model_weights', ((3, 4), [[0.0, 0.25, 0.5, 0.75], [1.0, 1.25, 1.5, 1.75], [2.0, 2.25, 2.5, 2.75]])),
                     ('model_flags', ((3, 1), [[0.0], [2.0], [1073741824.0]]))]}


@pytest.mark.parametrize("product", list(SAVED))
def test_saved_file_holds_what_the_separate_savers_wrote(product, tmp_path):
    path = str(tmp_path / f"{product}.mat")
    getattr(io, f"save_{product}")(path, _saver_inputs()[product], processed_file="p.mat", multi_dla=np.float64(1))
    got = _saved(path)
    assert [name for name, _ in got] == [name for name, _ in SAVED[product]]
    for (name, have), (_, want) in zip(got, SAVED[product]):
        assert have == want, name
