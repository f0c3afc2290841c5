"""The sample generator on the GPU (csrc/sample_kernels.hpp, gp_dla_detection_amd/samples.py; DESIGN.md
4.15) against tests/sample_restatement.py: scrambled Halton points bit for bit against exact
rationals, the density estimate, the fitted quadratic, the cumulative table against adaptive
quadrature, the drawn samples against a bracketing root finder, and the file it writes driving both
sweeps and run_dr12q --multi.

Tolerances: the KDE 1e-12 relative (exponent arguments reach ~550, so one ulp of argument is ~1e-13
of a term); the fit 1e-10 (the restatement's raw-t Vandermonde has condition ~1e6); F, Z_lls, Z_dla
1e-12 (quad runs at epsabs 1e-13); |F_ref(x) - u| <= 1e-11 at every sample, ten times quad's own
floor of 8e-13; positions 1e-11 / p + 1e-12.
Observed on an MI355X: bandwidth identical, KDE 4.4e-16, fit 5.9e-14, F 1.2e-14, Z_lls / Z_dla 1e-14,
|F_ref(x) - u| 1.0e-13 over 10^4 samples, positions at 1% of their bound."""
import numpy as np
import pytest

import sample_restatement as R
from gp_dla_detection_amd import _lib, io, samples, synthetic
from gp_dla_detection_amd.parameters import MultiParameters

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def catalogue():
    return R.make_catalogue()


@pytest.fixture(scope="module")
def ref_priors(catalogue):
    """The restated priors, computed once: single (alpha 0.9), multi (0.97), LLS."""
    return dict(single=R.Prior(catalogue, 0.9), multi=R.Prior(catalogue, 0.97), lls=R.Prior(catalogue, lls=True))


def gpu_prior(catalogue, kind):
    if kind == "single":
        return samples.fit_nhi_prior(catalogue, samples.SampleParameters.single())
    return samples.fit_nhi_prior(catalogue, samples.SampleParameters.multi(), lls=(kind == "lls"))


# ---------------------------------------------------------------------------------------------
# Halton
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("first,num", [(0, 17), (255, 4), (2 ** 31 + 5, 4)])
def test_halton_is_bit_exact(first, num):
    got = samples.scrambled_halton(first, num)
    want = R.halton(first, num)
    assert got.shape == (num, 3) and got.tobytes() == want.tobytes()
    # the same range in two calls
    cut = num // 2
    parts = np.concatenate([samples.scrambled_halton(first, cut), samples.scrambled_halton(first + cut, num - cut)])
    assert parts.tobytes() == got.tobytes()


def test_halton_known_answers():
    h = samples.scrambled_halton(0, 4)
    assert (h[0] == 0.0).all()   # index 0 is the origin
    assert list(h[1:, 1]) == [2 / 3, 1 / 3, 2 / 9] and h[1, 2] == 4 / 5 and list(h[1:, 0]) == [0.5, 0.25, 0.75]
    seven = samples.scrambled_halton(1, 6, bases=(7,))[:, 0]
    assert list(seven) == [4 / 7, 2 / 7, 6 / 7, 1 / 7, 5 / 7, 3 / 7]
    assert samples.scrambled_halton(2 ** 32 - 1, 1).shape == (1, 3)   # the last index there is


# ---------------------------------------------------------------------------------------------
# KDE and fit
# ---------------------------------------------------------------------------------------------

def kde_catalogue(n, catalogue):
    if n == 6000:   # two chunks of the catalogue
        return 20 + np.random.default_rng(1).exponential(0.45, 6000)
    return catalogue[:n]


@pytest.mark.parametrize("G", [1, 1000])
@pytest.mark.parametrize("N", [2, 257, 6000])
def test_kde_matches_the_restatement(catalogue, N, G):
    v = kde_catalogue(N, catalogue)
    assert v.size == N
    x = np.array([21.3]) if G == 1 else R.fit_grid()
    want, h_ref = R.ksdensity(v, x), R.bandwidth(v)
    assert want.min() > 1e-290   # (no denormals: a relative tolerance means something)
    got, h = samples.kde(v, x, return_bandwidth=True)
    print(f"N={N} G={G}: bandwidth rel {abs(h - h_ref) / h_ref:.2e}, density rel {np.abs(got / want - 1).max():.2e}")
    assert abs(h - h_ref) <= 1e-15 * h_ref
    assert np.all(np.abs(got - want) <= 1e-12 * want)
    # a passed bandwidth is used as given
    got2, h2 = samples.kde(v, x, bandwidth=0.11, return_bandwidth=True)
    assert h2 == 0.11 and np.all(np.abs(got2 - R.ksdensity(v, x, 0.11)) <= 1e-12 * R.ksdensity(v, x, 0.11))
    if G == 1000:   # a grid point's value does not depend on where the launch puts it
        assert samples.kde(v, x[637:638])[0] == got[637]


def test_kde_refusals(catalogue):
    with pytest.raises(_lib.GpdlaError, match="median absolute deviation") as e:
        samples.kde(np.full(10, 20.5), [20.0, 21.0])
    assert e.value.code == -1
    assert samples.kde(np.full(10, 20.5), [20.5], bandwidth=0.1)[0] == pytest.approx(1 / (0.1 * np.sqrt(2 * np.pi)), rel=1e-14)
    # a catalogue so far from the fit grid that its density underflows there: the log fit is undefined
    with pytest.raises(_lib.GpdlaError, match="cannot be fitted") as e:
        samples.fit_nhi_prior(catalogue - 15.0)
    assert e.value.code == -1


def test_fit_matches_the_restatement(catalogue, ref_priors):
    p = samples.fit_nhi_prior(catalogue)
    ref = ref_priors["single"]
    x = ref.x
    c0, c1, c2 = p.coeff
    s = x - p.centre
    worst = np.abs(c0 + s * (c1 + s * c2) - np.polyval(ref.f, x)).max()
    print(f"fit: max |polyval_gpu - polyval_ref| on the grid {worst:.2e}; Z rel {abs(p.Z / ref.Z - 1):.2e}")
    assert p.centre == 21.0 and worst <= 1e-10
    assert np.abs(np.polyval(p.polyfit_coefficients(), x) - np.polyval(ref.f, x)).max() <= 1e-9
    assert abs(p.Z - ref.Z) <= 1e-12
    assert (p.alpha, p.uniform_min, p.uniform_max, p.lower) == (0.9, 20.0, 23.0, 20.0) and np.isnan(p.flat_below)


# ---------------------------------------------------------------------------------------------
# F and the normalisers
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["single", "multi", "lls"])
def test_cdf_matches_adaptive_quadrature(catalogue, ref_priors, kind):
    ref = ref_priors[kind]
    p = gpu_prior(catalogue, kind)
    lower = ref.lower
    pts = [lower, 19.5, 20.0, R.LLS_BREAK, 23.0, 25.0, np.nextafter(23.0, 0), np.nextafter(23.0, 30), lower + 1e-9, 24.999]
    x = np.concatenate([pts, np.random.default_rng(3).uniform(lower, 25.0, 64 - len(pts))])
    assert x.size == 64
    F = p.cdf(x)
    want = np.array([ref.cdf(t) for t in x])
    print(f"{kind}: max |F - quad| {np.abs(F - want).max():.2e}; F(25) - 1 = {F[5] - 1:.2e}")
    assert np.abs(F - want).max() <= 1e-12
    assert p.cdf(lower) == 0.0 and p.cdf(lower - 1.0) == 0.0 and p.cdf(26.0) == F[5]
    # the density: the exponent is held to 1e-10 on the fit grid (above); at 25 it is extrapolated four
    # half-widths of the grid from its centre, where a quadratic's coefficient errors weigh up to 16 times more
    d = p.pdf(x)
    want_d = np.array([ref.pdf(t) for t in x])
    print(f"{kind}: max relative density error {np.abs(d / want_d - 1).max():.2e}")
    assert np.all(np.abs(d - want_d) <= 16e-10 * want_d)


def test_lls_normalisers(catalogue, ref_priors):
    out = samples.generate_dla_samples(catalogue, multi=True, lls=True, num=4)
    ref = ref_priors["lls"]
    z_lls, z_dla = ref.cdf(20.0) - ref.cdf(19.5), ref.cdf(23.0) - ref.cdf(20.0)
    print(f"Z_lls {out['Z_lls']:.15f} (ref {z_lls:.15f}), Z_dla {out['Z_dla']:.15f} (ref {z_dla:.15f})")
    assert abs(out["Z_lls"] - z_lls) <= 1e-12 and abs(out["Z_dla"] - z_dla) <= 1e-12
    assert abs(out["Z_lls"] - 0.4821) < 1e-4 and abs(out["Z_dla"] - 0.5176) < 1e-4
    assert out["alpha"] == 0.97   # the scalars saved are those of the DLA samples (generate_dla_samples_multi.m:59-61)


# ---------------------------------------------------------------------------------------------
# samples
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [1, 257, 10000])
def test_samples_solve_the_restated_equation(catalogue, ref_priors, S):
    """F_ref at EVERY returned log_nhi against the sample's own u.  Positions against the bracketing root
    finder: every sample for S = 1 and 257; for S = 10000 every 16th sample, every sample above the
    uniform range and the one of smallest density (a root finder run per sample is what costs)."""
    ref = ref_priors["single"]
    out = samples.generate_dla_samples(catalogue, lls=True, num=S)
    seq = R.halton(0, S)
    x = out["log_nhi_samples"]
    assert sorted(out) == sorted(["offset_samples", "log_nhi_samples", "nhi_samples", "lls_log_nhi_samples",
                                  "lls_nhi_samples", "Z_lls", "Z_dla", "alpha", "uniform_min_log_nhi",
                                  "uniform_max_log_nhi", "fit_min_log_nhi", "fit_max_log_nhi"])
    assert all(out[k].shape == (S,) for k in out if k.endswith("_samples"))
    assert out["offset_samples"].tobytes() == seq[:, 0].tobytes()
    assert x[0] == 20.0   # u = 0: fit_min exactly
    assert np.all((x >= 20.0) & (x <= 25.0))
    F = np.array([ref.cdf(t) for t in x])
    print(f"S={S}: max |F_ref(x) - u| {np.abs(F - seq[:, 1]).max():.2e}")
    assert np.abs(F - seq[:, 1]).max() <= 1e-11
    dens = np.array([ref.pdf(t) for t in x])
    if S == 10000:
        assert np.count_nonzero(x > 23.0) == 5 and abs(dens.min() - 1.6e-4) < 1e-5
        check = np.unique(np.concatenate([np.arange(0, S, 16), np.flatnonzero(x > 23.0), [int(np.argmin(dens))]]))
    else:
        check = np.arange(S)
    worst = 0.0
    for i in check:
        x_ref = ref.inverse(seq[i, 1], bracket=(x[i] - 1e-8, x[i] + 1e-8))
        bound = 1e-11 / ref.pdf(x_ref) + 1e-12
        worst = max(worst, abs(x[i] - x_ref) / bound)
        assert abs(x[i] - x_ref) <= bound, (i, x[i], x_ref)
    print(f"S={S}: worst |x - x_ref| / bound {worst:.2e} over {check.size} samples")
    # nhi within 2 ulp of 10 ** log_nhi
    want = 10.0 ** x
    assert np.all(np.abs(out["nhi_samples"] - want) <= 2 * np.spacing(want))
    l = out["lls_log_nhi_samples"]
    assert np.all((l >= 19.5) & (l < 20.0))
    assert l.tobytes() == (19.5 + (20.0 - 19.5) * seq[:, 2]).tobytes()
    wl = 10.0 ** l
    assert np.all(np.abs(out["lls_nhi_samples"] - wl) <= 2 * np.spacing(wl))


def test_a_supplied_sequence_is_all_the_samples_depend_on(catalogue):
    S = 257
    base = samples.generate_dla_samples(catalogue, multi=True, lls=True, num=S)
    order = np.random.default_rng(8).permutation(S)
    seq = samples.scrambled_halton(0, S)[order]
    a = samples.generate_dla_samples(catalogue, multi=True, lls=True, sequence=seq)
    b = samples.generate_dla_samples(catalogue, multi=True, lls=True, sequence=seq, first_index=1000)
    for k in ("offset_samples", "log_nhi_samples", "nhi_samples", "lls_log_nhi_samples", "lls_nhi_samples"):
        assert a[k].tobytes() == base[k][order].tobytes(), k
        assert b[k].tobytes() == a[k].tobytes(), k
    # the ends of the unit interval, and two columns without the LLS outputs
    ends = samples.generate_dla_samples(catalogue, sequence=np.array([[0.0, 0.0], [1.0, 1.0], [0.5, 0.999999999]]))
    assert list(ends["log_nhi_samples"][:2]) == [20.0, 25.0] and 23.0 < ends["log_nhi_samples"][2] < 25.0
    assert "lls_nhi_samples" not in ends
    with pytest.raises(_lib.GpdlaError, match="third column"):
        samples.generate_dla_samples(catalogue, lls=True, sequence=np.full((3, 2), 0.5))


# ---------------------------------------------------------------------------------------------
# the file drives the sweeps
# ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fileset(tmp_path_factory, catalogue):
    d = tmp_path_factory.mktemp("samples_run")
    fs = synthetic.write_file_set(str(d / "in"), num_quasars=6, num_samples=256, empty_quasar=None)
    fs["generated"] = str(d / "generated_samples.mat")
    smp = samples.generate_dla_samples(catalogue, multi=True, lls=True, num=256)
    io.save_dla_samples(fs["generated"], smp)
    fs["generated_dict"] = smp
    return fs


def test_generated_file_drives_both_sweeps(fileset):
    import gp_dla_detection_amd as gp
    fs = fileset
    smp = io.load_dla_samples(fs["generated"])
    for k, v in smp.items():
        assert v.tobytes() == fs["generated_dict"][k].tobytes(), k
    Z = io.load_sample_normalisers(fs["generated"])
    assert Z == (fs["generated_dict"]["Z_lls"], fs["generated_dict"]["Z_dla"])
    sel = np.flatnonzero(fs["test_ind"])
    spectra = [fs["spectra"][i] for i in sel]
    out = gp.process_qsos(fs["model"], smp, spectra, prior_catalog=fs["prior"])
    assert np.all(np.isfinite(out["p_dlas"])) and np.all(np.isfinite(out["sample_log_likelihoods_dla"]))
    np.testing.assert_allclose(out["p_dlas"] + out["p_no_dlas"], 1.0, rtol=0, atol=1e-12)
    p = MultiParameters(max_dlas=2)
    z = fs["catalog"]["z_qsos"][sel]
    lp = gp.dla_existence_prior_multi(fs["prior"]["z_qsos"], fs["prior"]["dla_ind"], z, Z[0], Z[1], p)
    multi = gp.process_qsos_multiple_dlas_meanflux(fs["model"], smp, spectra, lp, params=p)
    assert np.all(np.isfinite(multi["model_posteriors"]))
    np.testing.assert_allclose(multi["model_posteriors"].sum(axis=1), 1.0, rtol=0, atol=1e-12)


def test_run_dr12q_multi_takes_the_normalisers_from_the_file(fileset, tmp_path):
    from gp_dla_detection_amd import run_dr12q
    fs = fileset
    p = fs["paths"]

    def argv(samples_file, out, *extra):
        return ["--preloaded", p["preloaded"], "--catalog", p["catalog"], "--learned", p["learned"], "--samples",
                samples_file, "--prior", p["prior"], "--out", str(out), "--name", "gen", "--multi", "--max-dlas", "2",
                *extra]

    run_dr12q.main(argv(fs["generated"], tmp_path / "from_file"))
    Z = io.load_sample_normalisers(fs["generated"])
    run_dr12q.main(argv(fs["generated"], tmp_path / "flags", "--z-lls", repr(Z[0]), "--z-dla", repr(Z[1])))
    run_dr12q.main(argv(fs["generated"], tmp_path / "other", "--z-lls", "0.31", "--z-dla", "0.69"))
    name = "processed_qsos_multi_meanfluxgen_summary.mat"
    a, b, c = (io.loadmat73(str(tmp_path / d / name))["model_posteriors"] for d in ("from_file", "flags", "other"))
    assert np.all(np.isfinite(a)) and a.tobytes() == b.tobytes()
    assert a.tobytes() != c.tobytes()   # explicit flags win
    np.testing.assert_allclose(a.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    with pytest.raises(ValueError, match="needs Z_lls and Z_dla"):   # synthetic's file carries none
        run_dr12q.main(argv(p["samples"], tmp_path / "none"))
    with pytest.raises(ValueError, match="needs Z_lls and Z_dla"):   # one flag alone is not a pair
        run_dr12q.main(argv(fs["generated"], tmp_path / "half", "--z-lls", "0.4"))


def test_command_line_writes_the_file(catalogue, tmp_path):
    np.savez(tmp_path / "log_nhis.npz", log_nhis=catalogue)
    out = str(tmp_path / "dla_samples.mat")
    samples.main([str(tmp_path / "log_nhis.npz"), out, "--multi", "--lls", "--num", "64"])
    smp, direct = io.load_dla_samples(out), samples.generate_dla_samples(catalogue, multi=True, lls=True, num=64)
    for k, v in smp.items():
        assert v.tobytes() == direct[k].tobytes(), k
    assert io.load_sample_normalisers(out) == (direct["Z_lls"], direct["Z_dla"])
