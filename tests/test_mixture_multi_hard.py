"""The exact fixture of the all-model mixture products (tests/golden/exact_mixture_multi_hard.npz, made by
tests/golden/make_exact_mixture_multi_hard.py from tests/mixture_multi_hard_cases.py) on the CPU: the stored inputs, base
indices and rows are what the builders form today, both fp64 restatement forms stay within the cap of the 50-digit values on
every (class, row, mixture, product), the stored values are reproduced from the stored inputs, a never-drawn slot keeps its
sample out of every exact sum, and the comparison the GPU test uses notices three in-bounds mutations of the restatement.
Figures of the committed fixture are in LABBOOK.md ("All-model mixture products against exact arithmetic")."""
import numpy as np
import pytest

import continuum_hard_cases as CH
import hard_conditioning_cases as H
import mixture_multi_hard_cases as XH

NAMES = [H.class_name(cls) for cls in XH.CLASSES]


@pytest.fixture(scope="module")
def fixture(golden):
    return XH.load_fixture(golden)


@pytest.fixture(scope="module")
def hard(golden):
    return H.load_fixture(golden)


_restated = {}


def restated(fixture, cls, form="woodbury", mutation=None):
    """({(row, mixture number): products}, {row: moments}) of the restatement on the stored inputs, once per class, form and
    mutation ("nu32", "short", "row0")"""
    key = (cls, form, mutation)
    if key not in _restated:
        e = fixture[H.class_name(cls)]
        inp = XH.stored_inputs(e)
        bsi = e["base_sample_inds"]
        full = XH.with_products(inp, bsi, mutation if mutation in ("short", "row0") else None)
        nu = inp["nu"].astype(np.float32).astype(np.float64) if mutation == "nu32" else None
        per_sample = XH.restatement_samples(full, form, nu)
        eff = {row: XH.effective_rows(XH.stored_rows(e, row), bsi) for row in XH.ROWS}
        products = {(row, m): XH.restatement_products(full, per_sample, eff[row], XH.MIXTURES[m]) for row, m in XH.COMBOS}
        moments = {row: XH.restatement_moments(full, eff[row], XH.MIXTURES[0]) for row in XH.MOMENT_ROWS} if cls in XH.MOMENT_CLASSES else {}
        _restated[key] = (products, moments)
    return _restated[key]


def test_fixture_holds_every_class_row_and_mixture(fixture):
    assert sorted(fixture) == sorted(NAMES)
    for cls in XH.CLASSES:
        e = fixture[H.class_name(cls)]
        k = cls[2]
        for row, m in XH.COMBOS:
            exact = XH.stored_exact(e, row, m)
            assert set(exact) == set(CH.MC_PRODUCTS + CH.PR.PRODUCTS)
            assert exact["coef_mean"].shape == (k,) and exact["coef_cov_between"].shape == (k * (k + 1) // 2,)
            assert all(exact[n].shape == (H.N_PIX,) for n in CH.PR.PRODUCTS + CH.MC_PRODUCTS[1:2])
            assert np.array_equal(np.isnan(exact["noise_var"]), ~e["kept"])
            assert all(np.isfinite(exact[n]).all() for n in exact if n != "noise_var")
            assert (exact["continuum_var"] >= exact["continuum_var_between"]).all() and (exact["continuum_var_between"] >= 0).all()
            assert (exact["flux_var_between"] >= 0).all() and (exact["flux_var_within"] >= 0).all()
        for row in XH.MOMENT_ROWS if cls in XH.MOMENT_CLASSES else ():
            mo = XH.stored_moments(e, row)
            assert set(mo) == set(XH.MOMENTS) and mo["mean_absorption_models"].shape == (XH.MD, H.N_PIX)
            assert all(np.isfinite(v).all() and (v >= 0).all() for v in mo.values())
        assert not any(key.startswith("moments/") for key in e) or cls in XH.MOMENT_CLASSES


def test_fixture_is_no_larger_than_the_largest_exact_fixture():
    import glob
    import os
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    others = [os.path.getsize(p) for p in glob.glob(os.path.join(here, "exact_*.npz")) if os.path.basename(p) != XH.FIXTURE]
    assert os.path.getsize(os.path.join(here, XH.FIXTURE)) <= max(others)


@pytest.mark.parametrize("cls", XH.CLASSES, ids=H.class_name)
def test_stored_inputs_are_in_sync(cls, fixture, hard, oracle):
    """bit for bit what H.build_case, XH.inputs, XH.base_sample_inds and XH.weight_rows form today"""
    e = fixture[H.class_name(cls)]
    case = H.build_case(cls)
    inp = XH.inputs(oracle, case)
    assert set(inp) == set(XH.INPUT_KEYS)
    for key, v in inp.items():
        np.testing.assert_array_equal(v, e[key], err_msg=f"{H.class_name(cls)} {key}")
    np.testing.assert_array_equal(XH.base_sample_inds(cls[0], case["samples"]), e["base_sample_inds"])
    rows = XH.weight_rows(hard[H.class_name(cls)], case["samples"]["offset_samples"])
    for comp in XH.SAMPLED:
        for row in XH.ROWS:
            np.testing.assert_array_equal(rows[comp][row], e[f"row/{comp}/{row}"], err_msg=f"{comp} {row}")
    assert int(e["kept"].sum()) == H.N_PIX - 5 and e["profiles_dla"].shape == (H.S, H.N_PIX)


def test_base_indices_are_what_they_claim(fixture):
    for cls in XH.CLASSES:
        e = fixture[H.class_name(cls)]
        bsi, C = e["base_sample_inds"].astype(np.int64), e["profiles_dla"]
        assert bsi.shape == (XH.MD - 1, H.S) and bsi.min() == 0 and bsi.max() <= H.S
        assert all((bsi[a] != bsi[b]).sum() > H.S // 2 for a in range(3) for b in range(a))      # the rows differ
        for i in XH.FOURTH:                                                                     # a fourth power
            assert (bsi[:, i] == i + 1).all()
            np.testing.assert_array_equal(XH.product_profiles(C, bsi, 4)[i], C[i] * C[i] * C[i] * C[i])
        assert sorted(zip(*np.nonzero(bsi.T == 0))) == sorted((i, slot - 2) for slot, i in XH.ZEROS)
        if cls[0] != "saturated":
            continue
        case = H.build_case(cls)
        u = XH.least_absorbed(case["samples"])
        chains = XH.chains(case["samples"])
        deep = range(8, H.NUM_PLACED)
        print(f"saturated: least absorbed sample {u}, log N_HI {case['samples']['log_nhi_samples'][u]:.2f}, deepest pixel {C[u].min():.4f}, "
              f"{int((C[u] > 0.99).sum())} of {H.N_PIX} pixels absorbed by less than 1 %")
        assert (C[u] > 0.99).mean() > 0.75 and C[u].min() > 0.25 and all(  # one shallow line: as unabsorbed as the sample box allows
np.asarray(case["samples"]["log_nhi_samples"])[j] == 23.0 for j in (0, 2, 4, 6))
        for i in deep:           # every DEEP trough meets a log N_HI = 23 trough and the least absorbed sample in one chain
            assert (bsi[:, i] - 1).tolist() == list(chains[i]) and u in chains[i] and set(chains[i]) & {0, 2, 4, 6}
            assert (C[i] == 0).any(), i                                                 # exactly 0 inside
        denormal = [int(((C[i] > 0) & (C[i] < 2.3e-308)).sum()) for i in deep]
        print(f"saturated: denormal rim pixels of the DEEP samples {denormal}")
        assert sum(n > 0 for n in denormal) >= 2
        A4 = XH.product_profiles(C, bsi, 4)
        rim = [int(((C[i] > 0) & (C[i] < 2.3e-308) & (A4[i] == 0)).sum()) for i in deep]
        print(f"saturated: denormal rim pixels of the DEEP samples that the four-fold product takes to 0: {rim}")
        assert all(np.isfinite(A4).all() and (A4 >= 0).all() for _ in (0,))


def test_rows_are_what_they_claim(fixture):
    for cls in XH.CLASSES:
        e = fixture[H.class_name(cls)]
        bsi = e["base_sample_inds"]
        for comp in XH.SAMPLED:
            rows = {row: e[f"row/{comp}/{row}"] for row in XH.ROWS}
            n = {row: CH.n_eff(v) for row, v in rows.items()}
            assert abs(n["top8_flat"] - 8) < 1e-12 and abs(n["adjacent_pair"] - 2) < 1e-12 and abs(n["flat"] - H.S) < 1e-10
            assert 1 < n["near_one_hot"] < 1 + 3e-6
            live = {row: CH.R.weights(v) > 0 for row, v in rows.items()}
            assert all(((v == CH.DEAD) == ~live[row]).all() for row, v in rows.items())
            pair = np.sort(np.argsort(np.argsort(e["z_dlas"]))[live["adjacent_pair"]])
            assert pair[1] - pair[0] == 1                                  # neighbours in z_DLA order
        tops = [tuple(np.flatnonzero(e[f"row/{comp}/top8_flat"] == 0)) for comp in XH.SAMPLED]
        assert len(set(tops)) == len(tops)                                 # every component's row sits elsewhere
        eff = XH.effective_rows(XH.stored_rows(e, "flat"), bsi)
        print(f"{H.class_name(cls)}: live samples of the flat row " + ", ".join(f"{c} {int((CH.R.weights(v) > 0).sum())}" for c, v in eff.items()))


@pytest.mark.parametrize("cls", XH.CLASSES, ids=H.class_name)
def test_both_restatement_forms_stay_under_the_cap(cls, fixture):
    """A condition on the choice of inputs, not a measurement: on every (row, mixture, product) both fp64 forms are within
    RESTATEMENT_CAP of the exact value in the scaled measure (and per pixel, relatively, on the three products bounded away
    from 0), so that 10 x the Woodbury form's error is a bound that still says something; the moments likewise."""
    e, name = fixture[H.class_name(cls)], H.class_name(cls)
    for form in ("woodbury", "dense"):
        products, moments = restated(fixture, cls, form)
        worst = 0.0
        for (row, m), got in products.items():
            for n, e_rest, e_got, tol in CH.figures(got, XH.stored_exact(e, row, m), got):
                assert e_got <= e_rest            # the family's figure is the largest of its products'
                worst = max(worst, e_got)
                assert e_got <= CH.RESTATEMENT_CAP, (name, form, row, m, n, e_got)
        for row, got in moments.items():
            for n, e_rest, e_got, tol in XH.moment_figures(got, XH.stored_moments(e, row), got):
                assert e_got <= e_rest <= XH.TOL_MOMENTS / CH.TOL_FACTOR, (name, row, n, e_got)     # the floor is the bound
        print(f"{name}: worst {form} restatement error {worst:.3e}")


def test_stored_exact_values_are_reproduced_and_fifty_digits_are_enough(fixture):
    """``correlated-multi-k20-l3`` ``adjacent_pair`` under the mixture of the gathered models (the null model and two samples
    each of DLA(2), DLA(3) and DLA(4)): the 50-digit values round to the stored ones, and 30 digits agree with them to 1e-20."""
    import mpmath as mp
    cls = XH.CLASSES[0]
    e = fixture[H.class_name(cls)]
    inp = XH.stored_inputs(e)
    bsi = e["base_sample_inds"]
    full = XH.with_products(inp, bsi)
    eff = XH.effective_rows(XH.stored_rows(e, "adjacent_pair"), bsi)
    p = XH.MIXTURES[1]
    pairs = XH.live_pairs(eff, p)
    assert len(pairs) == 6 and {c for c, _ in pairs} == {"dla2", "dla3", "dla4"}
    raw = {}
    for dps in (30, 50):
        args = (CH.rows_of(inp), inp["mu_all"], inp["M_all"])
        per_sample = {"null": [CH.exact_sample(*args, np.ones(H.N_PIX), inp["kept"], dps)], **{c: {} for c in XH.SAMPLED}}
        for c, i in pairs:
            per_sample[c][i] = CH.exact_sample(*args, full["profiles_" + c][i], inp["kept"], dps)
        raw[dps] = XH.exact_products(per_sample, eff, p, inp["mu_all"], inp["M_all"], dps, raw=True)
    with mp.workdps(60):
        worst = mp.mpf(0)
        for n in raw[50]:
            both = [(x, y) for x, y in zip(raw[30][n], raw[50][n]) if not mp.isnan(y)]
            worst = max(worst, max(abs(x - y) for x, y in both) / max(abs(y) for _, y in both))
    print(f"30 against 50 digits: worst relative difference {float(worst):.2e}")
    assert worst < 1e-20
    stored = XH.stored_exact(e, "adjacent_pair", 1)
    for n, v in raw[50].items():
        np.testing.assert_array_equal(np.array([float(x) for x in v]), stored[n], err_msg=n)
    for row in XH.MOMENT_ROWS[:2]:
        eff = XH.effective_rows(XH.stored_rows(e, row), bsi)
        again = XH.exact_moments(full, eff, XH.MIXTURES[0])
        for n, v in XH.stored_moments(e, row).items():
            np.testing.assert_array_equal(again[n], v, err_msg=f"{row} {n}")


def test_never_drawn_slots_keep_their_samples_out_of_every_exact_sum(fixture):
    """A sample with base index 0 in slot j has weight 0 in DLA(j) .. DLA(4) whatever its placed log-likelihood says, and
    keeps it in the models before: it is among no (row, mixture)'s live pairs there, the restatement that leaves it out
    meets the exact values (the cap test), and one that draws the slot (index 1 in its place) misses the ``flat`` ones by
    far more than the bound."""
    for cls in XH.CLASSES:
        e, name = fixture[H.class_name(cls)], H.class_name(cls)
        bsi = e["base_sample_inds"]
        for row in XH.ROWS:
            placed = XH.stored_rows(e, row)
            eff = XH.effective_rows(placed, bsi)
            for slot, i in XH.ZEROS:
                for n in range(1, XH.MD + 1):
                    comp = f"dla{n}"
                    if n >= slot:
                        assert np.isnan(eff[comp][i]) and (comp, i) not in XH.live_pairs(eff, np.ones(6))
                    else:
                        assert eff[comp][i] == placed[comp][i]
                    if row == "flat":
                        assert placed[comp][i] == 0.0          # the placed row would give it 1 / 65 of the weight
            assert all(np.array_equal(eff[c], placed[c], equal_nan=True) for c in ("sub_dla", "dla1"))
        drawn = np.where(bsi == 0, 1, bsi)
        inp = XH.stored_inputs(e)
        full = XH.with_products(inp, drawn)
        per_sample = XH.restatement_samples(full, "woodbury")
        rows = XH.stored_rows(e, "flat")
        for m in range(3):
            exact, rest = XH.stored_exact(e, "flat", m), restated(fixture, cls)[0]["flat", m]
            got = XH.restatement_products(full, per_sample, XH.effective_rows(rows, drawn), XH.MIXTURES[m])
            bad = CH.failures(name, CH.figures(got, exact, rest))
            print(f"{name} flat mixture {m}: with the never-drawn slots drawn {len(bad)} figures fail")
            assert bad, (name, m)


def test_profile_parity_outweighs_the_restatement_on_one_sample(fixture):
    """Why the ``near_one_hot`` row is printed, not asserted, on the GPU.  Its one live sample of DLA(4) makes e_restatement one
    draw of one inversion.  The device forms its own Voigt profiles, each held to PARITY = 2e-13 of the oracle's; with the four
    stored profiles of that sample moved by up to that much (seeded, 200 draws) the restatement's Sigma moves by ten times
    its own error on ``correlated``, 31 lines, and a Cholesky inverse of the SAME B -- the device's algorithm -- is no worse
    than the LU inverse.  The inputs decide that figure, not the arithmetic."""
    PARITY = 2e-13
    rng = np.random.default_rng(31)
    for cls in XH.CLASSES:
        e, name = fixture[H.class_name(cls)], H.class_name(cls)
        inp, bsi, k = XH.stored_inputs(e), e["base_sample_inds"], cls[2]
        i = int(np.argmax(e["row/dla4/near_one_hot"]))
        s, C, kept = XH.RM.slots(bsi, XH.MD, i), inp["profiles_dla"], inp["kept"]
        a = XH.product_profiles(C, bsi, XH.MD)[i]
        exact = CH.exact_sample(CH.rows_of(inp), inp["mu_all"], inp["M_all"], a, kept)
        Sig = np.zeros((k, k))
        Sig[np.tril_indices(k)] = [float(x) for x in exact["Sig"]]
        Sig = Sig + np.tril(Sig, -1).T
        y, mu, M, omega2, nu = CH.rows_of(inp)
        d = a[kept] ** 2 * omega2 + nu
        B = np.eye(k) + M.T @ ((a[kept] ** 2 / d)[:, None] * M)
        X = np.linalg.inv(np.linalg.cholesky(B))
        e_lu, e_chol = np.abs(np.linalg.inv(B) - Sig).max(), np.abs(X.T @ X - Sig).max()
        moved = []
        for _ in range(200):
            ap = np.ones_like(a)
            for sj in s:
                ap = ap * (C[sj] + PARITY * rng.uniform(-1, 1, a.size))
            moved.append(np.abs(CH.MR.sample_woodbury(y, mu, M, omega2, nu, ap[kept])[1] - Sig).max())
        print(f"{name} sample {i} slots {s}: cond(B_i) {np.linalg.cond(B):.1e}; |Sigma - exact| LU {e_lu:.2e}, Cholesky {e_chol:.2e}; "
              f"profiles moved by {PARITY:.0e}: median {np.median(moved):.2e}, largest {max(moved):.2e}")
        assert e_chol <= 10 * e_lu + 1e-15
        if cls == ("correlated", "single", 20, 31):
            assert np.median(moved) > 5 * e_lu and max(moved) > 10 * e_lu


MUTATIONS = {"nu32": "noise variances rounded to float32", "short": "the slot loop stops at n - 1",
             "row0": "every slot gathered from row 0 of base_sample_inds"}


@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_comparison_notices_an_in_bounds_mutation(mutation, fixture):
    """The restatement itself passes its own bound on every (class, row, mixture); under each mutation -- all of them read
    and write in bounds and leave every value finite -- the helper the GPU test asserts with reports failures in every class,
    and on the moments too where the mutation reaches the profiles."""
    for cls in XH.CLASSES:
        e, name = fixture[H.class_name(cls)], H.class_name(cls)
        products, moments = restated(fixture, cls)
        broken, broken_moments = restated(fixture, cls, mutation=mutation)
        bad, worst = [], 0.0
        for (row, m), rest in products.items():
            exact = XH.stored_exact(e, row, m)
            assert CH.failures(name, CH.figures(rest, exact, rest)) == []
            assert all(np.isfinite(v[np.isfinite(exact[n])]).all() for n, v in broken[row, m].items())
            figs = CH.figures(broken[row, m], exact, rest)
            bad += CH.failures(f"{name} {row} {m}", figs)
            worst = max(worst, max(CH.ratio(e_got, tol) for _, _, e_got, tol in figs))
        print(f"{name}: {MUTATIONS[mutation]}: {len(bad)} figures fail; worst error / tolerance {worst:.3g}")
        assert bad, (name, mutation, worst)
        for row, rest in moments.items():
            exact = XH.stored_moments(e, row)
            assert XH.moment_failures(name, XH.moment_figures(rest, exact, rest)) == []
            if mutation != "nu32":
                assert XH.moment_failures(name, XH.moment_figures(broken_moments[row], exact, rest)), (name, row, mutation)
