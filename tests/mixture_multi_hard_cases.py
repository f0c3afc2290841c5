"""The marginal continuum, the predictive flux and the absorption moments over ALL models of a multi-DLA run (DESIGN.md
4.25, 4.21) where the arithmetic is hard (plain module beside continuum_hard_cases.py, whose exact evaluation, error measure,
bound and fixture storage these are: the generator tests/golden/make_exact_mixture_multi_hard.py, test_mixture_multi_hard.py
and test_gpu_mixture_multi_hard.py import it, nothing else does).

What is new against continuum_hard_cases.py is the profile of a sample: for model DLA(n) the running product
A_{n,i} = Prod_j c_{s_j(i)} of up to four gathered profiles (``product_profiles``), multiplied in slot order in fp64 from the
stored ``oracle.voigt`` profiles, as the contract of include/gpdla.h says; the 50-digit value is taken AT that product, the
input the restatement sees.

    classes     CLASSES: four of H.CLASSES (their quasar, model, noise and samples), every one run with max_dlas = 4; the two
                "multi" ones with the mean-flux rows, the two "single" ones with the plain rows (31 lines; k = 40)
    base        ``base_sample_inds``: [3, S], seeded, 1-based; fourth powers (FOURTH), in ``saturated`` chains through the
                DEEP troughs, a log N_HI = 23 trough and the least absorbed sample (CHAINS), three never-drawn slots (ZEROS)
    rows        ROWS, one kind for all five sampled components of a call: ``CH.weight_rows`` of the stored exact table of the
                sub-DLA model and of DLA(1); of DLA(2..4), and of the sub-DLA model where the parent holds no exact table
                for it, the same construction on the stored exact DLA row under a fixed seeded permutation (ROW_SEED).  No
                ``sweep`` kind: the parent's only table of a model n >= 2 was swept with other base indices.
    mixtures    MIXTURES, (null, sub-DLA, DLA(1..4)); COMBOS pairs them with the rows: the third meets ``flat`` and
                ``near_one_hot`` only, and ``near_one_hot`` (one live sample a model: printed on the GPU, not asserted) only it

The figures, the bound max(10 x e_restatement, 1e-12) and the cap on the choice of inputs are continuum_hard_cases.py's.
The absorption moments solve no matrix: one family, the same rule, the floor TOL_MOMENTS.
"""
from __future__ import annotations

import numpy as np

import continuum_hard_cases as CH
import hard_conditioning_cases as H
import model_spectra_multi_restatement as RM
import model_spectra_restatement as R

MD = 4
CLASSES = (
    ("correlated", "multi", 20, 3),         # mean-flux rows; k_mc_contract_multi<4,4,32>
    ("saturated", "multi", 20, 3),
    ("correlated", "single", 20, 31),       # plain rows; the run-time line count in the slot loop
    ("correlated", "single", 40, 3),        # plain rows; k_mc_contract_multi<1,14,64>
)
MOMENT_CLASSES = CLASSES[:2]
FIXTURE = "exact_mixture_multi_hard.npz"
CONTINUUM = "continuum:"       # a reference into the resolved exact_continuum_hard*.npz, beside CH.PARENT
SAMPLED = ("sub_dla",) + tuple(f"dla{n}" for n in range(1, MD + 1))
COMPONENTS = ("null",) + SAMPLED
ROWS = ("top8_flat", "adjacent_pair", "flat", "near_one_hot")
MIXTURES = ((0.1, 0.15, 0.3, 0.2, 0.15, 0.1),
            (0.2, 0.0, 0.0, 0.3, 0.2, 0.3),      # the gathered models carry the result
            (0.0, 0.0, 0.0, 0.0, 0.0, 1.0))      # four-fold products alone
COMBOS = tuple((row, m) for row in ROWS[:3] for m in (0, 1)) + (("flat", 2), ("near_one_hot", 2))
MOMENT_ROWS = ROWS[:3]         # with MIXTURES[0]
BASE_SEED, ROW_SEED = 4177, 5200
FOURTH = (20, 41)              # samples whose four slots all name the sample itself
ZEROS = ((2, 13), (3, 30), (4, 52))      # (slot, sample): never drawn; weight 0 from model DLA(slot) on
TOL_MOMENTS = 1e-11            # tests/test_gpu_model_spectra.py's (test_gpu_mixture_multi_hard.py asserts the identity)
MOMENTS = ("mean_absorption_models", "var_absorption_models", "mean_absorption_lls", "var_absorption_lls",
           "expected_absorption", "expected_var_absorption")

# (stratum, k) -> what had to be chosen so that the Woodbury-form restatement stays within CH.RESTATEMENT_CAP of the exact
# value on every stored (class, row, mixture); the GPU is never consulted.  Empty: with the parent's own tuning
# (H.TUNING: flux factor and noise draw per class) and the seeds above, the first ones tried, the cap holds everywhere.
TUNING: dict = {}


def meanflux_of(cls) -> bool:
    return cls[1] == "multi"


def least_absorbed(samples) -> int:
    """the sample of smallest column density that ``H.sample_table`` did not place"""
    return H.NUM_PLACED + int(np.argmin(np.asarray(samples["log_nhi_samples"])[H.NUM_PLACED:]))


def chains(samples) -> dict:
    """``saturated``: {sample: its slots 2..4, 0-based}.  8 .. 11 are the DEEP troughs (exactly 0 inside, denormal on the
    rim), 0, 2, 4 and 6 the log N_HI = 23 troughs of the three lines, u the least absorbed sample."""
    u = least_absorbed(samples)
    return {8: (0, u, 10), 9: (u, 2, 6), 10: (6, 11, u), 11: (4, u, 8), 0: (8, u, 2), 6: (9, 1, u)}


def base_sample_inds(stratum: str, samples) -> np.ndarray:
    """[MD - 1, S], 1-based, 0 = never drawn"""
    bsi = np.random.default_rng(BASE_SEED).integers(1, H.S + 1, size=(MD - 1, H.S)).astype(np.uint32)
    for i in FOURTH:
        bsi[:, i] = i + 1
    if stratum == "saturated":
        for i, slots in chains(samples).items():
            bsi[:, i] = np.asarray(slots) + 1
    for slot, i in ZEROS:
        bsi[slot - 2, i] = 0
    return bsi


def product_profiles(profiles, bsi, n: int, mutation: str | None = None) -> np.ndarray:
    """[S, n_u]: A_{n,i} = c_i c_{s_2(i)} .. c_{s_n(i)}, multiplied in slot order in fp64; a row of ones where a slot was never
    drawn (weight 0: any finite row does).  ``mutation``: "short" -- the slot loop stops at n - 1; "row0" -- every slot
    is gathered from row 0 of ``bsi``."""
    C = np.asarray(profiles, dtype=np.float64)
    A = np.ones_like(C)
    for i in range(C.shape[0]):
        s = RM.slots(bsi, n, i)
        if s is None:
            continue
        if mutation == "short":
            s = s[:max(1, n - 1)]
        elif mutation == "row0":
            s = [i] + [int(bsi[0][i]) - 1] * (n - 1)
        a = C[s[0]]
        for sj in s[1:]:
            a = a * C[sj]
        A[i] = a
    return A


def with_products(inp: dict, bsi, mutation: str | None = None) -> dict:
    """the inputs with ``profiles_dla<n>``, n = 1 .. MD, beside ``profiles_sub_dla``"""
    out = dict(inp)
    for n in range(1, MD + 1):
        out[f"profiles_dla{n}"] = product_profiles(inp["profiles_dla"], bsi, n, mutation)
    return out


def inputs(oracle, case) -> dict:
    """``CH.inputs`` and, for a class whose parent has no sub-DLA table, the sub-DLA profiles formed the same way"""
    inp = CH.inputs(oracle, case)
    if "profiles_sub_dla" not in inp:
        g = R.grid(oracle, case["model"], case["spectrum"])
        nhi = case["samples"]["lls_nhi_samples"]
        inp["profiles_sub_dla"] = np.stack([oracle.voigt(g["pad"], inp["z_dlas"][i], nhi[i], case["cls"][3]) for i in range(H.S)])
    return inp


INPUT_KEYS = CH.INPUT_KEYS + ("profiles_sub_dla", "profiles_dla")


def row_permutation(comp: str) -> np.ndarray:
    return np.random.default_rng(ROW_SEED + SAMPLED.index(comp)).permutation(H.S)


def weight_rows(hard_entry: dict, offset_samples) -> dict:
    """{component: {row kind: [S] host log-likelihood row}} from the parent fixture's exact tables; depends on no run"""
    out = {}
    for comp in SAMPLED:
        if comp == "sub_dla" and "exact_lls" in hard_entry:
            ll = hard_entry["exact_lls"]
        elif comp == "dla1":
            ll = hard_entry["exact_dla"]
        else:
            ll = np.asarray(hard_entry["exact_dla"])[row_permutation(comp)]
        rows = CH.weight_rows(ll, offset_samples)
        out[comp] = {row: rows[row] for row in ROWS}
    return out


def effective_rows(rows: dict, bsi) -> dict:
    """{component: row} with a NaN where a slot of the sample was never drawn: what carries weight"""
    return {comp: (np.array(v) if comp == "sub_dla" else RM.effective_row(v, bsi, int(comp[3:]))) for comp, v in rows.items()}


def host_tables(rows: dict, bsi) -> dict:
    """the tables of one call, [1, ...]: the rows AS PLACED -- a finite entry on a never-drawn slot is the library's to ignore"""
    return dict(sample_log_likelihoods_dla=np.stack([rows[f"dla{n}"] for n in range(1, MD + 1)])[None],
                base_sample_inds=np.asarray(bsi, dtype=np.uint32)[None], sample_log_likelihoods_lls=np.asarray(rows["sub_dla"])[None])


def live_pairs(rows_eff: dict, p) -> list:
    """[(component, sample)] that a (row, mixture) evaluates"""
    return [(comp, int(i)) for comp, pm in zip(SAMPLED, p[1:]) if pm > 0 for i in np.flatnonzero(R.weights(rows_eff[comp]) > 0)]


# ---------------------------------------------------------------- the restatement on stored inputs

def restatement_samples(inp_products: dict, form: str, nu=None) -> dict:
    return CH.restatement_samples(inp_products, SAMPLED, form, nu)


def restatement_products(inp_products: dict, per_sample: dict, rows_eff: dict, p) -> dict:
    return CH.restatement_products(inp_products, per_sample, rows_eff, p, components=COMPONENTS)


def exact_products(per_sample: dict, rows_eff: dict, p, mu_all, M_all, dps: int = CH.DPS, raw: bool = False) -> dict:
    return CH.exact_products(per_sample, rows_eff, p, mu_all, M_all, dps, raw, components=COMPONENTS)


# ---------------------------------------------------------------- the absorption moments

def restatement_moments(inp_products: dict, rows_eff: dict, p) -> dict:
    """Per model mean = Sum w A and var = Sum w (A - mean)^2 as ``RM.moments_multi`` forms them, the sub-DLA model's, and
    ``RM.model_average`` of them (the weights ``p`` as given: this entry does not normalise them)"""
    mean, var = {}, {}
    for comp in SAMPLED:
        w = R.weights(rows_eff[comp])
        A = inp_products["profiles_" + comp]
        mean[comp] = w @ A
        var[comp] = w @ (A - mean[comp]) ** 2
    mb, m2 = zip(*(RM.absorbed_moments(mean[comp], var[comp]) for comp in SAMPLED))
    expected, variance, undefined = RM.model_average(p, mb, m2, [False] * len(SAMPLED))
    assert not undefined
    return dict(mean_absorption_models=np.stack([mean[c] for c in SAMPLED[1:]]), var_absorption_models=np.stack([var[c] for c in SAMPLED[1:]]),
                mean_absorption_lls=mean["sub_dla"], var_absorption_lls=var["sub_dla"], expected_absorption=expected,
                expected_var_absorption=variance)


def exact_moments(inp_products: dict, rows_eff: dict, p, dps: int = CH.DPS) -> dict:
    """the same at ``dps`` digits from the same fp64 profiles and rows, rounded to fp64 at the very end"""
    import mpmath as mp
    with mp.workdps(dps):
        n_u = inp_products["profiles_sub_dla"].shape[1]
        mean, var = {}, {}
        for comp in SAMPLED:
            live, w = CH.exact_weights(rows_eff[comp], dps)
            A = [[mp.mpf(x) for x in inp_products["profiles_" + comp][i].tolist()] for i in live]
            mean[comp] = [mp.fsum(wi * a[px] for wi, a in zip(w, A)) for px in range(n_u)]
            var[comp] = [mp.fsum(wi * (a[px] - mean[comp][px]) ** 2 for wi, a in zip(w, A)) for px in range(n_u)]
        eb, eb2 = [mp.mpf(0)] * n_u, [mp.mpf(0)] * n_u
        for comp, pm in zip(SAMPLED, p[1:]):
            pm = mp.mpf(float(pm))
            mb = [1 - x for x in mean[comp]]
            eb = [x + pm * b for x, b in zip(eb, mb)]
            eb2 = [x + pm * (v + b * b) for x, v, b in zip(eb2, var[comp], mb)]
        out = dict(mean_absorption_models=[mean[c] for c in SAMPLED[1:]], var_absorption_models=[var[c] for c in SAMPLED[1:]],
                   mean_absorption_lls=mean["sub_dla"], var_absorption_lls=var["sub_dla"], expected_absorption=[1 - x for x in eb],
                   expected_var_absorption=[b - a * a for a, b in zip(eb, eb2)])
        return {name: np.array([[float(x) for x in r] for r in v] if isinstance(v[0], list) else [float(x) for x in v])
                for name, v in out.items()}


def moment_figures(got: dict, exact: dict, restatement: dict) -> list:
    """[(label, e_restatement of the family, e_got, tolerance)]: one family, ``CH.error``, floor TOL_MOMENTS"""
    fam = max(CH.error(restatement[n], exact[n]) for n in MOMENTS)
    tol = max(CH.TOL_FACTOR * fam, TOL_MOMENTS)
    return [(n, fam, CH.error(got[n], exact[n]), tol) for n in MOMENTS]


def moment_failures(label: str, figs: list) -> list:
    return [f"{label} {n}: error {e:.3e} > {tol:.3e} = max(10 x {er:.3e}, {TOL_MOMENTS:.0e})" for n, er, e, tol in figs if not e <= tol]


# ---------------------------------------------------------------- the fixture

def load_fixture(golden) -> dict:
    """{class name: {key: array}}; "<key>@" holds where an array stored once lives: a full key of this file, CH.PARENT + a
    full key of exact_hard_conditioning.npz, or CONTINUUM + <class name>/<key> of the resolved exact_continuum_hard*.npz"""
    parent = golden(H.FIXTURE)
    continuum = CH.load_fixture(golden)
    z = golden(FIXTURE)
    flat = {full: z[full] for full in z.files}
    out = {}
    for full, v in flat.items():
        name, key = full.split("/", 1)
        if key.endswith("@"):
            ref = str(v)
            if ref.startswith(CH.PARENT):
                v = parent[ref[len(CH.PARENT):]]
            elif ref.startswith(CONTINUUM):
                v = continuum[ref[len(CONTINUUM):].split("/", 1)[0]][ref[len(CONTINUUM):].split("/", 1)[1]]
            else:
                v = flat[ref]
        out.setdefault(name, {})[key.rstrip("@")] = v
    return out


def stored_inputs(entry: dict) -> dict:
    return {key: entry[key] for key in INPUT_KEYS}


def stored_rows(entry: dict, row: str) -> dict:
    return {comp: entry[f"row/{comp}/{row}"] for comp in SAMPLED}


def stored_exact(entry: dict, row: str, mix: int) -> dict:
    prefix = f"exact/{row}/{mix}/"
    return {key[len(prefix):]: v for key, v in entry.items() if key.startswith(prefix)}


def stored_moments(entry: dict, row: str) -> dict:
    prefix = f"moments/{row}/"
    return {key[len(prefix):]: v for key, v in entry.items() if key.startswith(prefix)}
