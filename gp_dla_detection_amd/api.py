"""Python host side of the MI355X inference sweep: the reference's call surface over libgpdla.so.

Mirrors, name for name, what a user of jibanCat/gp_dla_detection calls on this path:

=========================================  =====================================================
reference                                  here
=========================================  =====================================================
``voigt(lambdas, z, N, num_lines)`` MEX    :func:`voigt`                      (voigt.c:253-304)
``log_mvnpdf_low_rank(y, mu, M, d)``       :func:`log_mvnpdf_low_rank`        (log_mvnpdf_low_rank.m:5)
DLA-existence prior of the driver          :func:`dla_existence_prior`        (process_qsos.m:122-131)
``process_qsos`` script                    :func:`process_qsos`               (process_qsos.m:88-244)
``process_qsos_multiple_dlas_meanflux``    :func:`process_qsos_multiple_dlas_meanflux`
                                                                              (multi_dlas/...m:141-510)
=========================================  =====================================================

plus :class:`Context` / :class:`Batch` for callers that keep spectra resident in HBM (what
``bench.py`` times, and what the multi-GPU driver in :mod:`.distributed` uses).  NumPy arrays and
PyTorch-ROCm tensors are staging only; all arithmetic happens in the HIP kernels.
"""
from __future__ import annotations

import ctypes as C
from contextlib import closing
from types import SimpleNamespace

import numpy as np

from . import _lib, grid_fields
from .parameters import MultiParameters, Parameters

_dp = C.POINTER(C.c_double)
_i64p = C.POINTER(C.c_int64)
_i32p = C.POINTER(C.c_int32)


def _f64(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(_dp)


def _absorber_fields(rq, absorbers, n: int, keep: list, what: str):
    """Absorber lists ``(offsets [n + 1], z_dlas, log_nhis)`` in CSR form (or None) into the absorber_* fields of
    a request; the arrays the fields point at are appended to ``keep``."""
    if absorbers is None:
        return
    a_off, a_z, a_ln = absorbers
    a_off = np.ascontiguousarray(a_off, dtype=np.int64).reshape(-1)
    if a_off.size != n + 1:
        raise _lib.GpdlaError(-1, f"absorber offsets: {a_off.size} entries for {n} {what}")
    a_z, a_n = _f64(a_z)[0].reshape(-1), 10.0 ** _f64(a_ln)[0].reshape(-1)
    keep += [a_off, a_z, a_n]
    rq.absorber_offsets, rq.absorber_z, rq.absorber_nhi = a_off.ctypes.data_as(_i64p), a_z.ctypes.data_as(_dp), a_n.ctypes.data_as(_dp)


def _config(params: Parameters) -> _lib.Config:
    lib = _lib.load()
    cfg = _lib.Config()
    lib.gpdla_default_config(C.byref(cfg))
    for name in ("min_lambda", "max_lambda", "lya_wavelength", "lyman_limit", "pixel_spacing",
                 "max_z_cut", "min_z_cut", "width", "num_lines"):
        setattr(cfg, name, getattr(params, name))
    for name in ("max_dlas", "num_forest_lines", "min_z_separation", "prev_tau_0", "prev_beta",
                 "rng_seed", "first_quasar_index", "contraction_precision", "multi_profile_bytes",
                 "record_pool_bytes"):
        if hasattr(params, name):
            setattr(cfg, name, getattr(params, name))
    return cfg


# ----------------------------------------------------------------------------------------------
# stand-alone surfaces
# ----------------------------------------------------------------------------------------------

def voigt(lambdas, z, N, num_lines: int = 31, device: int = 0) -> np.ndarray:
    """``profile = voigt(lambdas, z, N[, num_lines])`` -- voigt.c:253-304.

    Returns ``numel(lambdas) - 6`` values (the MEX trims ``width = 3`` pixels per side, :271).
    ``num_lines`` defaults to 31 like the MEX (:16, :266)."""
    lib = _lib.load()
    lam, lp = _f64(lambdas)
    if lam.size <= 6:
        raise _lib.GpdlaError(-1, "lambdas must have more than 2*width = 6 entries")
    out = np.empty(lam.size - 6)
    _lib.check(lib.gpdla_voigt(lp, lam.size, float(z), float(N), int(num_lines),
                               out.ctypes.data_as(_dp), int(device)))
    return out


def log_mvnpdf_low_rank(y, mu, M, d, device: int = 0) -> float:
    """``log_p = log_mvnpdf_low_rank(y, mu, M, d)`` -- log N(y; mu, M M' + diag(d))
    (log_mvnpdf_low_rank.m:5-34).  ``M`` is (n, k).  Raises GpdlaError(-4) where MATLAB's
    ``chol`` would throw (:24)."""
    lib = _lib.load()
    y, yp = _f64(y)
    mu, mup = _f64(mu)
    d, dp = _f64(d)
    Mf = np.asfortranarray(M, dtype=np.float64)
    if Mf.ndim != 2 or Mf.shape[0] != y.size or mu.size != y.size or d.size != y.size:
        raise _lib.GpdlaError(-1, "shape mismatch: y, mu, d are n-vectors and M is n x k")
    out = C.c_double()
    _lib.check(lib.gpdla_log_mvnpdf_low_rank(yp, mup, Mf.ctypes.data_as(_dp), dp, y.size,
                                             Mf.shape[1], C.byref(out), int(device)))
    return out.value


def prepare_prior(prior_z_qsos, prior_dla_ind, prior_z_dlas, params: Parameters | None = None) -> dict:
    """process_qsos.m:11-27: the training catalogue's (z_QSO, has-a-DLA) pairs behind the model
    prior, with a sightline's flag cleared when every one of its catalogued DLAs lies blueward of the
    quasar's Lyman limit -- ``observed_wavelengths(lya_wavelength, z_dla) <
    observed_wavelengths(lyman_limit, z_qso)`` (:21-25) -- where this search never looks.
    ``prior_z_dlas[i]`` is the list of DLA redshifts of sightline i (the cell of
    ``prior_catalog.z_dlas(dla_catalog_name)``); it is read only where ``prior_dla_ind[i]``.
    Returns ``dict(z_qsos, dla_ind)`` as :func:`process_qsos` takes for ``prior_catalog``."""
    p = params or Parameters()
    z = np.asarray(prior_z_qsos, dtype=np.float64).reshape(-1)
    ind = np.array(prior_dla_ind, dtype=bool).reshape(-1)
    if ind.size != z.size or len(prior_z_dlas) != z.size:
        raise ValueError("prior_z_qsos, prior_dla_ind and prior_z_dlas must have one entry per sightline")
    for i in np.flatnonzero(ind):
        z_dlas = np.atleast_1d(np.asarray(prior_z_dlas[i], dtype=np.float64))
        # MATLAB's `if (vector < scalar)` is true only when every element is
        if z_dlas.size and np.all(p.lya_wavelength * (1 + z_dlas) < p.lyman_limit * (1 + z[i])):
            ind[i] = False
    return dict(z_qsos=z, dla_ind=ind)


def dla_existence_prior(prior_z_qsos, prior_dla_ind, z_qsos, params: Parameters | None = None):
    """process_qsos.m:122-131: log p(DLA | z_QSO) and log p(no DLA | z_QSO) from the counts of
    training-catalog quasars with z < z_QSO + prior_z_qso_increase.  Host logic (SURVEY.md
    section 8a row A3)."""
    p = params or Parameters()
    pz = np.asarray(prior_z_qsos, dtype=np.float64)
    pd = np.asarray(prior_dla_ind, dtype=bool)
    z = np.atleast_1d(np.asarray(z_qsos, dtype=np.float64))
    order = np.argsort(pz, kind="stable")
    pz_sorted = pz[order]
    cum_dla = np.concatenate([[0], np.cumsum(pd[order])])
    num_quasars = np.searchsorted(pz_sorted, z + p.prior_z_qso_increase, side="left")  # strict <
    num_dlas = cum_dla[num_quasars]
    with np.errstate(divide="ignore", invalid="ignore"):
        log_dla = np.log(num_dlas.astype(np.float64)) - np.log(num_quasars.astype(np.float64))
        log_no = (np.log((num_quasars - num_dlas).astype(np.float64))
                  - np.log(num_quasars.astype(np.float64)))
    return log_no, log_dla


# ----------------------------------------------------------------------------------------------
# resident form
# ----------------------------------------------------------------------------------------------

class _DeviceArray:
    """Zero-copy view of library-owned HBM for torch.as_tensor (CUDA array interface)."""

    def __init__(self, ptr: int, shape, owner):
        self.__cuda_array_interface__ = {"shape": tuple(int(s) for s in shape), "typestr": "<f8",
                                         "data": (int(ptr), False), "version": 2}
        self._owner = owner  # keeps the batch alive


def spectra_to_csr(spectra):
    """The ragged cell arrays of preloaded_qsos.mat (preload_qsos.m:64-79) as flat CSR arrays."""
    sizes = [np.asarray(s["wavelengths"]).size for s in spectra]
    offsets = np.zeros(len(spectra) + 1, dtype=np.int64)
    np.cumsum(sizes, out=offsets[1:])
    cat = lambda key, dt: (np.concatenate([np.asarray(s[key], dtype=dt).ravel() for s in spectra])
                           if spectra else np.zeros(0, dt))
    return dict(offsets=offsets, wavelengths=cat("wavelengths", np.float64),
                flux=cat("flux", np.float64), noise_variance=cat("noise_variance", np.float64),
                pixel_mask=cat("pixel_mask", np.uint8),
                z_qsos=np.array([float(s["z_qso"]) for s in spectra], dtype=np.float64))


class Context:
    """A device + stream + the replicated GP model and DLA samples (gpdla_context)."""

    def __init__(self, device: int = 0, params: Parameters | None = None, stream=None):
        self.lib = _lib.load()
        self.device = int(device)
        self.params = params or Parameters()
        self._h = C.c_void_p()
        _lib.check(self.lib.gpdla_context_create(self.device, C.byref(self._h)))
        cfg = _config(self.params)
        _lib.check(self.lib.gpdla_context_set_config(self._h, C.byref(cfg)))
        if stream is not None:
            self.set_stream(stream)
        self.num_samples = 0
        self.has_lls_samples = False
        self.k = 0
        self.refine_points = None

    def set_stream(self, stream):
        """``stream``: a raw hipStream_t (int) or a torch.cuda.Stream."""
        ptr = getattr(stream, "cuda_stream", stream)
        _lib.check(self.lib.gpdla_context_set_stream(self._h, C.c_void_p(int(ptr) if ptr else None)))

    def set_model(self, model: dict):
        """Fields of learned_qso_model_*.mat (process_qsos.m:30-35)."""
        keep = []
        m = _model_struct(model, keep)
        _lib.check(self.lib.gpdla_context_set_model(self._h, C.byref(m)))
        self.k = int(m.k)

    def set_samples(self, samples: dict):
        """Fields of dla_samples.mat (process_qsos.m:38-40)."""
        keep = []
        s = _samples_struct(samples, keep)
        _lib.check(self.lib.gpdla_context_set_samples(self._h, C.byref(s)))
        self.num_samples = int(s.num_dla_samples)
        self.has_lls_samples = samples.get("lls_nhi_samples") is not None
        # scales of log N for Batch.parameter_summaries' correlation floor (DLA table, sub-DLA table)
        self._log_nhi_scale = [float(np.max(np.abs(samples["log_nhi_samples"]))) if samples.get("log_nhi_samples") is not None else np.nan,
                               float(np.max(np.abs(np.log10(samples["lls_nhi_samples"])))) if self.has_lls_samples else np.nan]

        # ranges of log N: the default log N axis of Batch.posterior_maps (DLA table, sub-DLA table)
        ln = samples.get("log_nhi_samples")
        ln = np.asarray(ln, dtype=np.float64) if ln is not None else np.log10(np.asarray(samples["nhi_samples"], dtype=np.float64))
        lls = np.log10(np.asarray(samples["lls_nhi_samples"], dtype=np.float64)) if self.has_lls_samples else np.array([np.nan])
        self._log_nhi_range = [(float(ln.min()), float(ln.max())), (float(lls.min()), float(lls.max()))]

    def set_refine_points(self, u=None, v=None, num: int | None = None):
        """The unit-square point set of :meth:`Batch.refine` (gpdla_context_set_refine_points): ``u`` and
        ``v`` in [0, 1), any number of them.  Without arguments: ``num`` (default: the number of DLA samples)
        RR2-scrambled Halton points of bases 2 and 3 from index 1 (:func:`refine.default_points`)."""
        from . import refine
        if u is None:
            u, v = refine.default_points(int(num) if num is not None else self.num_samples, self.device)
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(-1)
        v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
        if u.size != v.size:
            raise ValueError(f"{u.size} u for {v.size} v")
        _lib.check(self.lib.gpdla_context_set_refine_points(self._h, u.size, _lib.ptr(u), _lib.ptr(v)))
        self.refine_points = (u.copy(), v.copy())

    def set_timing(self, enabled: bool):
        _lib.check(self.lib.gpdla_context_set_timing(self._h, int(bool(enabled))))

    def last_sweep_ms(self) -> float:
        return float(self.lib.gpdla_context_last_sweep_ms(self._h))

    def synchronize(self):
        _lib.check(self.lib.gpdla_context_synchronize(self._h))

    def upload(self, spectra, log_priors_no_dla, log_priors_dla, log_priors_lls=None) -> "Batch":
        """Spectra + priors to HBM.  With ``log_priors_lls`` the batch is a multi-DLA batch
        (``log_priors_dla`` is then [nq, max_dlas]) and is swept with :meth:`Batch.process_multi`."""
        return Batch(self, spectra, log_priors_no_dla, log_priors_dla, log_priors_lls)

    def set_params(self, params: Parameters):
        """Replace the whole configuration.  Not while another thread uploads a batch of this
        context (the upload reads it): a pipeline sets the per-batch key of the multi-DLA resampling
        with :meth:`set_first_quasar_index` instead."""
        self.params = params
        cfg = _config(params)
        _lib.check(self.lib.gpdla_context_set_config(self._h, C.byref(cfg)))

    def set_first_quasar_index(self, index: int):
        """The global index of the next multi-DLA batch's first quasar (keys the Philox resampling,
        multi :467-472).  Safe beside a concurrent upload (gpdla_context_set_first_quasar_index)."""
        _lib.check(self.lib.gpdla_context_set_first_quasar_index(self._h, int(index)))

    def close(self):
        if self._h:
            self.lib.gpdla_context_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Batch:
    """A CSR batch of spectra resident in HBM together with its result tables (gpdla_batch)."""

    def __init__(self, ctx: Context, spectra, log_priors_no_dla, log_priors_dla, log_priors_lls=None):
        self.ctx = ctx
        self._h = C.c_void_p()
        self._refined = None   # (levels, refine points) of the last refine() of the current spectra
        self._fill(spectra, log_priors_no_dla, log_priors_dla, log_priors_lls)

    def reload(self, spectra, log_priors_no_dla, log_priors_dla, log_priors_lls=None):
        """Replace the batch's spectra in place (gpdla_batch_reload): device allocations are reused
        where large enough, so the batch slots of a pipeline allocate nothing in the steady state.
        The previous results must have been downloaded."""
        self._fill(spectra, log_priors_no_dla, log_priors_dla, log_priors_lls)

    def _fill(self, spectra, log_priors_no_dla, log_priors_dla, log_priors_lls):
        ctx = self.ctx
        self._refined = None
        self._multi_processed = False   # process_multi() has run on the current spectra
        csr = spectra if isinstance(spectra, dict) else spectra_to_csr(spectra)
        self._csr = csr                 # (references: predictive_flux(residuals=True) reads the flux and the mask)
        self.num_quasars = csr["z_qsos"].size
        self.num_pixels = int(csr["offsets"][-1] - csr["offsets"][0])
        self.num_samples = ctx.num_samples
        self.max_dlas = int(getattr(ctx.params, "max_dlas", 0)) if log_priors_lls is not None else 0
        keep = []

        def ptr(a, dt, ct):
            a = np.ascontiguousarray(a, dtype=dt)
            keep.append(a)
            return a.ctypes.data_as(C.POINTER(ct))

        lp_dla = np.asarray(log_priors_dla, dtype=np.float64)
        if self.max_dlas:
            lp_dla = lp_dla.reshape(self.num_quasars, self.max_dlas)
        sp = _lib.Spectra(
            self.num_quasars, ptr(csr["offsets"], np.int64, C.c_int64),
            ptr(csr["wavelengths"], np.float64, C.c_double), ptr(csr["flux"], np.float64, C.c_double),
            ptr(csr["noise_variance"], np.float64, C.c_double),
            ptr(csr["pixel_mask"], np.uint8, C.c_uint8), ptr(csr["z_qsos"], np.float64, C.c_double),
            ptr(log_priors_no_dla, np.float64, C.c_double), ptr(lp_dla, np.float64, C.c_double),
            ptr(log_priors_lls, np.float64, C.c_double) if self.max_dlas else None)
        if not self._h:
            _lib.check(ctx.lib.gpdla_batch_upload(ctx._h, C.byref(sp), C.byref(self._h)))
        else:
            _lib.check(ctx.lib.gpdla_batch_reload(ctx._h, self._h, C.byref(sp)))
        self.log_priors_no_dla = np.array(log_priors_no_dla, dtype=np.float64)
        self.log_priors_dla = np.array(lp_dla, dtype=np.float64)
        self.log_priors_lls = None if log_priors_lls is None else np.array(log_priors_lls, dtype=np.float64)

    def process(self):
        """Launch the sweep for every quasar of the batch (asynchronous on the context's stream)."""
        _lib.check(self.ctx.lib.gpdla_batch_process(self.ctx._h, self._h))

    _SINGLE_VECTORS = ("min_z_dlas", "max_z_dlas", "log_likelihoods_no_dla", "log_likelihoods_dla",
                       "log_posteriors_no_dla", "log_posteriors_dla", "p_no_dlas", "p_dlas",
                       "MAP_inds", "MAP_z_dlas", "MAP_log_nhis")  # MAP_*: generate_ascii_catalog.m:73-80

    @classmethod
    def empty_results(cls, nq: int, S: int, with_samples: bool = True) -> dict:
        """Host arrays for the variables process_qsos.m:236-244 saves, for ``nq`` quasars."""
        out = {name: np.full(nq, np.nan) for name in cls._SINGLE_VECTORS}
        out["model_posteriors"] = np.full((nq, 2), np.nan)
        out["status"] = np.zeros(nq, dtype=np.int32)
        out["log_priors_no_dla"] = np.full(nq, np.nan)
        out["log_priors_dla"] = np.full(nq, np.nan)
        if with_samples:  # every row is written by a download (the device table is NaN-prefilled)
            out["sample_log_likelihoods_dla"] = np.empty((nq, S))
        return out

    def download(self, with_samples: bool = True, out: dict | None = None, at: int = 0) -> dict:
        """Results under the field names process_qsos.m:236-244 saves.  ``out`` / ``at``: write this
        batch's rows into rows ``at .. at + num_quasars`` of arrays made by :meth:`empty_results`
        (a pipeline's one set of output arrays) instead of allocating."""
        nq = self.num_quasars
        if out is None:
            out, at = self.empty_results(nq, self.num_samples, with_samples), 0
        r = _lib.Results()
        for name, _ in _lib.Results._fields_:
            if name in out:
                ct = C.c_int32 if name == "status" else C.c_double
                view = out[name][at:at + nq]
                assert view.flags.c_contiguous and view.shape[0] == nq
                setattr(r, name, view.ctypes.data_as(C.POINTER(ct)))
        _lib.check(self.ctx.lib.gpdla_batch_download(self.ctx._h, self._h, C.byref(r)))
        out["log_priors_no_dla"][at:at + nq] = self.log_priors_no_dla
        out["log_priors_dla"][at:at + nq] = self.log_priors_dla
        return out

    def debug_prepared_rows(self, quasar: int = 0, multi: bool = False) -> np.ndarray:
        """Test hook (gpdla_debug_prepared_rows): the (y, mu, omega2, nu) rows of one quasar on the
        unmasked-range grid after the preparation kernel alone, [n_u, 4]."""
        cap = 8192
        rows = np.empty((cap, 4))
        n = C.c_int64()
        _lib.check(self.ctx.lib.gpdla_debug_prepared_rows(self.ctx._h, self._h, int(bool(multi)), int(quasar),
                                                          rows.ctypes.data_as(_dp), cap, C.byref(n)))
        return rows[: n.value].copy()

    # ---- fixed absorbers ----

    def set_fixed_absorbers(self, absorbers, min_z_separation: float | None = None, meanflux_rows: bool | None = None):
        """Condition this single-DLA batch on fixed absorbers (gpdla_batch_set_fixed_absorbers; the contract is in
        include/gpdla.h): ``absorbers`` is the CSR triple ``(offsets [nq + 1], z_dlas, log_nhis)`` that
        :func:`map_absorbers` returns, one list of at most 8 per quasar of the batch, or None to clear.  After it
        :meth:`process` and :meth:`refine` evaluate ONE MORE absorber given the listed ones, and
        ``log_likelihoods_no_dla`` is the likelihood of the listed ones alone.  ``min_z_separation``: default from
        the context's parameters (a :class:`MultiParameters`' own, else the multi-DLA driver's 3000 km/s);
        ``meanflux_rows``: the rows of the multi-DLA driver (default: whether the parameters are
        :class:`MultiParameters`).  The batch is unprocessed afterwards; :meth:`reload` clears."""
        lib, p = self.ctx.lib, self.ctx.params
        if absorbers is None:
            _lib.check(lib.gpdla_batch_clear_fixed_absorbers(self.ctx._h, self._h))
        else:
            off, z, ln = absorbers
            off = np.ascontiguousarray(off, dtype=np.int64).reshape(-1)
            if off.size != self.num_quasars + 1:
                raise _lib.GpdlaError(-1, f"absorber offsets: {off.size} entries for {self.num_quasars} quasars")
            z, ln = _f64(z)[0].reshape(-1), _f64(ln)[0].reshape(-1)
            sep = getattr(p, "min_z_separation", MultiParameters().min_z_separation) if min_z_separation is None else min_z_separation
            mf = isinstance(p, MultiParameters) if meanflux_rows is None else bool(meanflux_rows)
            _lib.check(lib.gpdla_batch_set_fixed_absorbers(self.ctx._h, self._h, off.ctypes.data_as(_i64p), z.ctypes.data_as(_dp),
                                                           ln.ctypes.data_as(_dp), float(sep), int(mf)))
        self._refined = None

    def debug_conditioned_rows(self, quasar: int = 0, meanflux_rows: bool = False):
        """Test hook (gpdla_debug_conditioned_rows): ``(rows [n_u, 4], M [n_u, k])`` of one quasar on its
        unmasked-range grid after the preparation kernel and, on a conditioned batch, the conditioning.
        ``meanflux_rows`` chooses the preparation of an unconditioned batch; a conditioned one uses its own."""
        cap = 8192
        rows, M = np.empty((cap, 4)), np.empty((cap, self.ctx.k))
        n = C.c_int64()
        _lib.check(self.ctx.lib.gpdla_debug_conditioned_rows(self.ctx._h, self._h, int(bool(meanflux_rows)), int(quasar),
                                                             rows.ctypes.data_as(_dp), M.ctypes.data_as(_dp), cap, C.byref(n)))
        return rows[: n.value].copy(), M[: n.value].copy()

    # ---- model spectra ----

    def unmasked_counts(self) -> np.ndarray:
        """n_u of every quasar: the stored pixels with rest wavelength in [min_lambda, max_lambda],
        masked or not -- the grid the per-pixel outputs of :meth:`model_spectra` live on."""
        n = np.zeros(self.num_quasars, dtype=np.int64)
        _lib.check(self.ctx.lib.gpdla_batch_unmasked_counts(self.ctx._h, self._h, n.ctypes.data_as(_i64p)))
        return n

    def _grid_product(self, name: str, rq, sel, st, shapes, *validate_args) -> dict:
        """Run the grid product ``name`` (gpdla_<name>_validate, then gpdla_batch_<name>) for request ``rq`` over the
        selection ``sel`` into the output struct ``st``: ``offsets`` and ``status`` plus one float64 array per entry
        of ``shapes(total)`` (field name -> shape; ``total`` = the grid pixels of the selection, the capacity)."""
        lib = self.ctx.lib
        # refused requests never reach the device
        _lib.check(getattr(lib, f"gpdla_{name}_validate")(C.byref(rq), self.num_quasars, self.num_samples,
                                                          int(self.ctx.has_lls_samples), *validate_args))
        total = int(self.unmasked_counts()[sel].sum())
        rq.capacity = total
        out = {"offsets": np.zeros(sel.size + 1, dtype=np.int64), "status": np.zeros(sel.size, dtype=np.int32)}
        st.offsets = out["offsets"].ctypes.data_as(_i64p)
        st.status = out["status"].ctypes.data_as(_i32p)
        for field, shape in shapes(total).items():
            out[field] = np.empty(shape)
            setattr(st, field, out[field].ctypes.data_as(_dp))
        _lib.check(getattr(lib, f"gpdla_batch_{name}")(self.ctx._h, self._h, C.byref(rq), C.byref(st)))
        return out

    def _grid_product_multi(self, name: str, rq, sel, st, shapes) -> dict:
        """:meth:`_grid_product` for the three ``*_multi`` entries: their validate entries also take the batch's ``max_dlas`` and
        whether it was processed, and their output structs carry ``model_flags [nsel]`` (uint32), returned last."""
        flags = np.zeros(sel.size, dtype=np.uint32)
        st.model_flags = flags.ctypes.data_as(C.POINTER(C.c_uint32))
        out = self._grid_product(name, rq, sel, st, shapes, self.max_dlas, int(self._multi_processed))
        out["model_flags"] = flags
        return out

    def model_spectra(self, selection=None, absorbers=None, weights=None, sub_dla: bool = False,
                      meanflux: bool | None = None, products=("map", "moments", "continuum")) -> dict:
        """What the fitted model looks like on the selected quasars (gpdla_batch_model_spectra), per
        pixel of each quasar's unmasked-range grid.

        ``selection``: quasar indices of the batch (default: all, in order).
        ``absorbers``: ``(offsets [nsel + 1], z_dlas, log_nhis)`` in CSR form, one list per SELECTED quasar
        (what :func:`map_absorbers` returns for the same quasars), at most 8 each; None: no absorbers.
        ``weights``: ``"resident"`` -- the batch's own sample log-likelihoods after :meth:`process` /
        :meth:`process_multi` (multi: model DLA(1), or the sub-DLA table with ``sub_dla``) -- or a
        host array ``[nsel, S]`` of them (a processed file needs no second sweep); None: no moments.
        ``"refined"``: the batch's refined table after :meth:`refine` -- the S' refine points mapped through each
        quasar's last box, weighted by its refined sample log-posteriors.  Posterior mass outside
        the last box is ignored, as by ``parameter_summaries(refined=True)``; not with ``sub_dla``; a quasar the
        refine pass did not take (or found unusable) gets NaN rows and ``SPECTRA_NOT_REFINED`` in ``status``.
        ``meanflux``: prepared rows of the mean-flux model (default: on for a multi-DLA batch).
        ``products``: any of ``"map"`` (``map_absorption``), ``"moments"`` (``mean_absorption``,
        ``var_absorption``), ``"continuum"`` (``continuum``, ``model_flux``: the posterior mean of the
        low-rank part of the GP under the listed absorbers -- the pixel-diagonal omega term predicts
        nothing at an unmeasured pixel and is left out).
        Returns ``offsets [nsel + 1]``, ``status [nsel]`` and the flat per-pixel arrays; quasar s of the
        selection owns ``[offsets[s], offsets[s + 1])`` (:func:`split_cells` cuts them up)."""
        sel = self._selection(selection)
        nsel = sel.size
        rq = _lib.ModelSpectraRequest()
        rq.num_selected = nsel
        rq.selection = sel.ctypes.data_as(_i64p)
        keep = [sel]
        _absorber_fields(rq, absorbers, nsel, keep, "selected quasars")
        bits = {"map": _lib.SPECTRA_MAP, "moments": _lib.SPECTRA_MOMENTS, "continuum": _lib.SPECTRA_CONTINUUM}
        products = [p for p in products if not (p == "moments" and weights is None)]
        rq.products = int(sum(bits[p] for p in set(products)))
        self._weights_source(rq, weights, "an array [nsel, S]", [("weights", "sample_log_likelihoods", weights)], nsel, keep)
        rq.sub_dla = int(bool(sub_dla))
        rq.meanflux = int(bool(self.max_dlas) if meanflux is None else bool(meanflux))
        return self._grid_product("model_spectra", rq, sel, _lib.ModelSpectra(), lambda total: {
            name: total for p in set(products) for name in grid_fields.names("model_spectra", options=(p,))})

    def _weights_source(self, rq, weights, forms: str, tables, nsel: int, keep: list):
        """``weights`` of a grid product into ``rq.weights_source``: ``"resident"``, ``"refined"``, None (no source), or host
        tables -- ``tables`` lists them as (what the error text calls it, field of the request, ``[nsel, S]`` or None); the
        arrays the request points into are appended to ``keep``.  ``forms``: the host forms the call takes, for the error text."""
        if isinstance(weights, str):
            if weights not in ("resident", "refined"):
                raise ValueError(f"weights: 'resident', 'refined', {forms} or None")
            rq.weights_source = _lib.SPECTRA_WEIGHTS_RESIDENT if weights == "resident" else _lib.SPECTRA_WEIGHTS_REFINED
        elif weights is not None:
            rq.weights_source = _lib.SPECTRA_WEIGHTS_HOST
            for what, field, w in tables:
                if w is not None:
                    w = np.ascontiguousarray(w, dtype=np.float64)
                    if w.shape != (nsel, self.num_samples):
                        raise _lib.GpdlaError(-1, f"{what} must be [nsel, S] = {(nsel, self.num_samples)}, got {w.shape}")
                    keep.append(w)
                    setattr(rq, field, w.ctypes.data_as(_dp))

    def _multi_tables(self, rq, tables, nsel: int, keep: list) -> int:
        """Fill ``tables_source`` and the three table pointers of a multi-model request from ``tables`` ("resident" or a
        dict of host tables, as :meth:`model_spectra_multi` takes them); the arrays the request points into are appended to
        ``keep``.  Returns the tables' ``max_dlas``."""
        S = self.num_samples
        if isinstance(tables, str):
            if tables != "resident":
                raise ValueError("tables: 'resident' or a dict of host tables")
            rq.tables_source = _lib.SPECTRA_WEIGHTS_RESIDENT
            return self.max_dlas
        rq.tables_source = _lib.SPECTRA_WEIGHTS_HOST
        dla = np.ascontiguousarray(tables["sample_log_likelihoods_dla"], dtype=np.float64)
        if dla.ndim != 3 or dla.shape[0] != nsel or dla.shape[2] != S:
            raise _lib.GpdlaError(-1, f"sample_log_likelihoods_dla must be [nsel, max_dlas, S] = ({nsel}, max_dlas, {S}), got {dla.shape}")
        md = dla.shape[1]
        keep.append(dla)
        rq.sample_log_likelihoods_dla = dla.ctypes.data_as(_dp)
        if tables.get("sample_log_likelihoods_lls") is not None:
            lls = np.ascontiguousarray(tables["sample_log_likelihoods_lls"], dtype=np.float64)
            if lls.shape != (nsel, S):
                raise _lib.GpdlaError(-1, f"sample_log_likelihoods_lls must be [nsel, S] = {(nsel, S)}, got {lls.shape}")
            keep.append(lls)
            rq.sample_log_likelihoods_lls = lls.ctypes.data_as(_dp)
        if tables.get("base_sample_inds") is not None:
            base = np.ascontiguousarray(tables["base_sample_inds"], dtype=np.uint32)
            if base.shape != (nsel, md - 1, S):
                raise _lib.GpdlaError(-1, f"base_sample_inds must be [nsel, max_dlas-1, S] = {(nsel, md - 1, S)}, got {base.shape}")
            keep.append(base)
            rq.base_sample_inds = base.ctypes.data_as(C.POINTER(C.c_uint32))
        return md

    def model_spectra_multi(self, selection=None, tables="resident", model_weights=None, models=None,
                            products=("models", "average"), meanflux: bool | None = None, sub_dla: bool = True) -> dict:
        """The per-pixel absorption of a multi-DLA run averaged over the samples of every model and over
        the models (gpdla_batch_model_spectra_multi; the definitions are in include/gpdla.h), on the grid
        and in the layout of :meth:`model_spectra`.

        ``tables``: ``"resident"`` -- the batch's own tables after :meth:`process_multi` -- or a dict with
        ``sample_log_likelihoods_dla [nsel, max_dlas, S]``, ``base_sample_inds [nsel, max_dlas-1, S]``
        (1-based, 0 = never drawn) and ``sample_log_likelihoods_lls [nsel, S]`` of the SELECTED quasars (a
        processed file needs no second sweep); ``max_dlas`` is then the tables', and the batch may be any.
        ``model_weights``: ``[nsel, 2 + max_dlas]`` as (null, sub-DLA, DLA(1..max_dlas)), or None: the
        resident ``model_posteriors`` (resident tables only).  A NaN row (the reference's early exit) gives
        NaN averages; :func:`renormalised_model_posteriors` makes weights that include such quasars.
        ``models``: ``(first, last)`` or one model number (default: all).  ``products``: ``"models"``
        (``mean_absorption_models`` / ``var_absorption_models [max_dlas, total]``, NaN outside ``models``, and,
        ``sub_dla``, ``mean_absorption_lls`` / ``var_absorption_lls``) and ``"average"``
        (``expected_absorption``, ``expected_var_absorption``).
        Returns those with ``offsets [nsel + 1]``, ``status [nsel]`` and ``model_flags [nsel]`` (bit n-1: model
        DLA(n) has no weight; bit 30: the sub-DLA model)."""
        rq = _lib.ModelSpectraMultiRequest()
        sel, md, keep = self._mixture_multi_request(rq, selection, tables, model_weights, meanflux)
        first, last = (1, md) if models is None else ((int(models), int(models)) if np.isscalar(models) else
                                                      (int(models[0]), int(models[-1])))
        rq.first_model, rq.last_model = first, last
        bits = {"models": _lib.SPECTRA_MULTI_MODELS, "average": _lib.SPECTRA_MULTI_AVERAGE}
        products = set(products)
        rq.products = int(sum(bits[p] for p in products))

        def shapes(total):
            shapes = {}
            if "models" in products:
                shapes.update(mean_absorption_models=(md, total), var_absorption_models=(md, total))
                if sub_dla:
                    shapes.update(mean_absorption_lls=(total,), var_absorption_lls=(total,))
            if "average" in products:
                shapes.update(expected_absorption=(total,), expected_var_absorption=(total,))
            return shapes
        out = self._grid_product_multi("model_spectra_multi", rq, sel, _lib.ModelSpectraMulti(), shapes)
        del keep
        return out

    # ---- marginal continuum ----

    def _mixture_request(self, rq, selection, weights, components, model_weights, meanflux):
        """Fill the fields the marginal-continuum and the predictive-flux requests share; returns (selection,
        the arrays the request points into)."""
        sel = self._selection(selection)
        nsel, S = sel.size, self.num_samples
        names = ("null", "sub_dla", "dla")
        components = tuple(components)
        if not components or any(c not in names for c in components):
            raise ValueError(f"components: a non-empty subset of {names}")
        listed = np.array([c in components for c in names])
        if model_weights is None:
            pw = np.tile(listed.astype(np.float64), (nsel, 1))
        else:
            pw = np.array(model_weights, dtype=np.float64)
            if pw.shape != (nsel, 3):
                raise _lib.GpdlaError(-1, f"model_weights must be [nsel, 3] = {(nsel, 3)}, got {pw.shape}")
            pw[:, ~listed] = 0.0
        pw = np.ascontiguousarray(pw)
        rq.num_selected = nsel
        rq.selection = sel.ctypes.data_as(_i64p)
        rq.model_weights = pw.ctypes.data_as(_dp)
        keep = [sel, pw]
        if weights is not None and not isinstance(weights, (str, dict)):
            sampled = [c for c in components if c != "null"]
            if len(sampled) != 1:
                raise ValueError("weights: one array serves one sampled component; pass {'dla': ..., 'sub_dla': ...}")
            weights = {sampled[0]: weights}
        tables = weights if isinstance(weights, dict) else {}
        self._weights_source(rq, weights, "an array [nsel, S], a dict of them",
                             [(f"weights[{name!r}]", field, tables.get(name)) for name, field in
                              (("dla", "sample_log_likelihoods_dla"), ("sub_dla", "sample_log_likelihoods_lls"))], nsel, keep)
        rq.meanflux = int(bool(self.max_dlas) if meanflux is None else bool(meanflux))
        return sel, keep

    @staticmethod
    def _coefficient_samples(weights_source: int, model_weights, num_samples: int, num_refine_points) -> int:
        """Rows per quasar of ``sample_coefficients``, by the library's own rule: the S' refine points where the request
        runs the DLA component on the refined table -- the refined source AND some row of the model weights (columns of
        unlisted components already zeroed) weighs the DLA column -- and the batch's S otherwise.  A refined source whose
        DLA column is 0 everywhere is evaluated on the first pass's tables, so its rows are S long."""
        pw = np.asarray(model_weights, dtype=np.float64)
        if weights_source == _lib.SPECTRA_WEIGHTS_REFINED and bool((pw[:, 2] > 0).any()):
            if num_refine_points is None:
                raise _lib.GpdlaError(_lib.ERR_INVALID_ARGUMENT, "the batch has not been refined")
            return int(num_refine_points)
        return int(num_samples)

    def marginal_continuum(self, selection=None, weights="resident", components=("dla",), model_weights=None,
                           meanflux: bool | None = None, sample_coefficients: bool = False) -> dict:
        """The GP continuum of the selected quasars averaged over the absorber posterior instead of
        conditioned on one absorber list (gpdla_batch_marginal_continuum; the definitions are in
        include/gpdla.h): its posterior mean and variance per pixel of each quasar's unmasked-range grid,
        in the CSR layout of :meth:`model_spectra`.

        ``components``: which of ``"null"`` (no absorber), ``"sub_dla"`` (the sub-DLA sample table) and
        ``"dla"`` (the DLA sample table; a multi-DLA batch: model DLA(1)) are mixed.
        ``model_weights``: ``[nsel, 3]`` in the order (null, sub-DLA, DLA) -- columns of components that are
        not listed are ignored -- or None: equal weights over the listed components.  Rows are non-negative,
        finite and of positive sum; each is normalised by its sum.  A component of weight exactly 0 is not
        evaluated.
        ``weights``: ``"resident"`` (the batch's tables after :meth:`process` / :meth:`process_multi`), a host
        array ``[nsel, S]`` of sample log-likelihoods when one sampled component is listed, or a dict
        ``{"dla": ..., "sub_dla": ...}`` of them.  ``"refined"``: the DLA component runs on the batch's refined table
        after :meth:`refine` -- the S' refine points mapped through each quasar's last box, weighted by its refined
        sample log-posteriors; the null and the sub-DLA component are unchanged (the sub-DLA table keeps
        its S samples).  Posterior mass outside the last box is ignored, as by ``parameter_summaries(refined=True)``.  A
        quasar whose DLA component carries weight and that the refine pass did not take (or found unusable) gets NaN rows
        and status ``SPECTRA_NOT_REFINED``; ``sample_coefficients`` is then ``[nsel, S', k]``.
        ``meanflux``: prepared rows of the mean-flux model (default: on for a multi-DLA batch).
        ``sample_coefficients``: also ``sample_coefficients [nsel, S, k]``, the coefficient mean of every
        sample of the ONE sampled component, NaN rows for samples of weight 0.
        Returns ``offsets``, ``status``, the flat per-pixel ``continuum_mean``, ``continuum_var`` (within +
        between) and ``continuum_var_between``, ``coef_mean [nsel, k]``, ``coef_cov_within`` and
        ``coef_cov_between`` ``[nsel, k (k + 1) / 2]`` (packed lower triangles, row by row).  The variance is
        that of the low-rank part of the GP: the pixel-diagonal omega term predicts nothing at an
        unmeasured pixel and is left out, as in ``continuum`` of :meth:`model_spectra`."""
        rq = _lib.MarginalContinuumRequest()
        sel, keep = self._mixture_request(rq, selection, weights, components, model_weights, meanflux)
        nsel, k = sel.size, self.ctx.k
        S = self._coefficient_samples(rq.weights_source, keep[1], self.num_samples,
                                      None if self.ctx.refine_points is None else int(self.ctx.refine_points[0].size))
        rq.sample_coefficients = int(bool(sample_coefficients))
        nb = k * (k + 1) // 2
        rows = {"coef_mean": (nsel, k), "coef_cov_within": (nsel, nb), "coef_cov_between": (nsel, nb)}
        if sample_coefficients:
            rows["sample_coefficients"] = (nsel, S, k)
        out = self._grid_product("marginal_continuum", rq, sel, _lib.MarginalContinuum(),
                                 lambda total: {**{name: total for name in MARGINAL_CONTINUUM_ARRAYS}, **rows})
        del keep
        return out

    # ---- posterior predictive flux ----

    def grid_flux(self, selection=None):
        """``(flux, kept)`` of the selected quasars on their unmasked-range grids, flat in the CSR layout of
        :meth:`model_spectra`, from the host copy of the uploaded spectra: the observed flux and whether the
        pixel is not masked."""
        sel = self._selection(selection)
        csr, p = self._csr, self.ctx.params
        off = np.asarray(csr["offsets"], dtype=np.int64)
        ys, ks = [], []
        for q in sel:
            sl = slice(off[q], off[q + 1])
            rest = np.asarray(csr["wavelengths"][sl], dtype=np.float64) / (1 + float(csr["z_qsos"][q]))
            inside = (rest >= p.min_lambda) & (rest <= p.max_lambda)
            ys.append(np.asarray(csr["flux"][sl], dtype=np.float64)[inside])
            ks.append(np.asarray(csr["pixel_mask"][sl])[inside] == 0)
        return (np.concatenate(ys) if ys else np.zeros(0)), (np.concatenate(ks) if ks else np.zeros(0, dtype=bool))

    def predictive_flux(self, selection=None, weights="resident", components=("dla",), model_weights=None,
                        meanflux: bool | None = None, residuals: bool = False) -> dict:
        """The posterior predictive flux of the selected quasars (gpdla_batch_predictive_flux; the definitions
        are in include/gpdla.h): per pixel of each quasar's unmasked-range grid, the mean and variance of the model
        flux -- absorption times GP continuum -- averaged over the absorber posterior and the models.  It is the
        curve to lay over the observed spectrum, with its error band; it is NOT the product of ``mean_absorption``
        and ``continuum_mean``, because the continuum coefficients move with the absorber.

        ``selection``, ``weights``, ``components``, ``model_weights``, ``meanflux``: as :meth:`marginal_continuum`
        (``weights="refined"`` included: the DLA component on the refined table, mass outside the last box ignored).
        Returns ``offsets``, ``status`` and the flat per-pixel ``flux_mean``, ``flux_var`` (within + between),
        ``flux_var_within`` (the GP's spread given the absorber), ``flux_var_between`` (the spread over absorbers
        and models) and ``noise_var`` (NaN on masked pixels).  ``flux_var`` is the variance of the low-rank,
        noise-free model flux, as ``continuum_var`` is; ``flux_var + noise_var`` is the variance of a replicate
        observation of the pixel (a new pixel-diagonal term and new noise under the same posterior).

        ``residuals``: also ``residual`` = (y - flux_mean) / sqrt(flux_var + noise_var) per pixel, NaN on masked
        pixels, and per quasar ``chi2`` (the sum of its squares over the kept pixels) and ``num_kept``.  This is the
        IN-SAMPLE replicate residual: the pixel's own flux is among the data the posterior was formed from, so
        it is conservative (residuals come out smaller than leave-one-out ones would); it is not a leave-one-out
        residual."""
        rq = _lib.PredictiveFluxRequest()
        sel, keep = self._mixture_request(rq, selection, weights, components, model_weights, meanflux)
        out = self._grid_product("predictive_flux", rq, sel, _lib.PredictiveFlux(),
                                 lambda total: {name: total for name in PREDICTIVE_FLUX_ARRAYS})
        del keep
        if residuals:
            y, kept = self.grid_flux(sel)
            out.update(predictive_residuals(out, y, kept))
        return out

    # ---- marginal continuum and predictive flux over all models of a multi-DLA run ----

    def _mixture_multi_request(self, rq, selection, tables, model_weights, meanflux):
        """Fill what the three multi-model requests (:meth:`model_spectra_multi` and the two mixtures) share: selection, tables,
        ``max_dlas``, model weights and ``meanflux``; returns (selection, max_dlas, the arrays the request points into)."""
        sel = self._selection(selection)
        nsel = sel.size
        rq.num_selected = nsel
        rq.selection = sel.ctypes.data_as(_i64p)
        keep = [sel]
        md = self._multi_tables(rq, tables, nsel, keep)
        rq.max_dlas = md
        if model_weights is not None:
            w = np.ascontiguousarray(model_weights, dtype=np.float64)
            if w.shape != (nsel, 2 + md):
                raise _lib.GpdlaError(-1, f"model_weights must be [nsel, 2 + max_dlas] = {(nsel, 2 + md)}, got {w.shape}")
            keep.append(w)
            rq.model_weights = w.ctypes.data_as(_dp)
        rq.meanflux = int(bool(self.max_dlas) if meanflux is None else bool(meanflux))
        return sel, md, keep

    def marginal_continuum_multi(self, selection=None, tables="resident", model_weights=None, meanflux: bool | None = None) -> dict:
        """:meth:`marginal_continuum` over ALL models of a multi-DLA run (gpdla_batch_marginal_continuum_multi; the
        definitions are in include/gpdla.h): the components are (null, sub-DLA, DLA(1), .., DLA(max_dlas)), and sample i
        of model DLA(n) absorbs with the product of the n profiles of its slots, gathered through ``base_sample_inds`` as
        :meth:`model_spectra_multi` gathers them.

        ``tables``: ``"resident"`` or the dict of host tables of :meth:`model_spectra_multi`.
        ``model_weights``: ``[nsel, 2 + max_dlas]`` as (null, sub-DLA, DLA(1..max_dlas)), each row normalised by its sum, or
        None: the resident ``model_posteriors`` (resident tables only).  A negative or infinite entry is refused; a row
        with a NaN (the reference's early exit) gives NaN rows and ``SPECTRA_AVERAGE_UNDEFINED`` in ``status`` --
        :func:`renormalised_model_posteriors` makes weights that include such quasars.
        Returns what :meth:`marginal_continuum` returns (no ``sample_coefficients``) and ``model_flags [nsel]``: bit n-1 --
        model DLA(n) carries weight for the quasar and its table row has none (NaN rows, status 0); bit 30: the sub-DLA
        table."""
        rq = _lib.MarginalContinuumMultiRequest()
        sel, _md, keep = self._mixture_multi_request(rq, selection, tables, model_weights, meanflux)
        nsel, k = sel.size, self.ctx.k
        nb = k * (k + 1) // 2
        rows = {"coef_mean": (nsel, k), "coef_cov_within": (nsel, nb), "coef_cov_between": (nsel, nb)}
        out = self._grid_product_multi("marginal_continuum_multi", rq, sel, _lib.MarginalContinuumMulti(),
                                       lambda total: {**{name: total for name in MARGINAL_CONTINUUM_ARRAYS}, **rows})
        del keep
        return out

    def predictive_flux_multi(self, selection=None, tables="resident", model_weights=None, meanflux: bool | None = None,
                              residuals: bool = False) -> dict:
        """:meth:`predictive_flux` over ALL models of a multi-DLA run (gpdla_batch_predictive_flux_multi): the components,
        ``tables``, ``model_weights`` and ``model_flags`` of :meth:`marginal_continuum_multi`, the arrays and the
        ``residuals`` of :meth:`predictive_flux`."""
        rq = _lib.PredictiveFluxMultiRequest()
        sel, _md, keep = self._mixture_multi_request(rq, selection, tables, model_weights, meanflux)
        out = self._grid_product_multi("predictive_flux_multi", rq, sel, _lib.PredictiveFluxMulti(),
                                       lambda total: {name: total for name in PREDICTIVE_FLUX_ARRAYS})
        del keep
        if residuals:
            y, kept = self.grid_flux(sel)
            out.update(predictive_residuals(out, y, kept))
        return out

    # ---- absorption distribution ----

    @staticmethod
    def _distribution_request(rq, thresholds, bins, levels, histogram, keep: list):
        """Fill what the two absorption-distribution requests ask of the reduction; returns ``shapes(total)`` of the arrays
        the call returns.  The arrays the request points into are appended to ``keep``."""
        thr = np.ascontiguousarray(() if thresholds is None else thresholds, dtype=np.float64).reshape(-1)
        lev = np.ascontiguousarray(() if levels is None else levels, dtype=np.float64).reshape(-1)
        keep += [thr, lev]
        rq.num_thresholds, rq.thresholds = thr.size, thr.ctypes.data_as(_dp)
        rq.num_levels, rq.levels = lev.size, lev.ctypes.data_as(_dp)
        rq.num_bins = int(bins) if (histogram or lev.size) else 0
        B = rq.num_bins

        def shapes(total):
            out = {"prob_below": (thr.size, total), "absorption_min": (total,), "absorption_max": (total,)}
            if lev.size:
                out["quantiles"] = (lev.size, total)
            if histogram:
                out["histogram"] = (B, total)
            return out
        return shapes

    def absorption_distribution(self, selection=None, weights="resident", components=("dla",), model_weights=None,
                                thresholds=(0.8,), bins: int = 64, levels=None, histogram: bool = False,
                                meanflux: bool | None = None) -> dict:
        """The per-pixel DISTRIBUTION of the absorption of the selected quasars over the absorber posterior and the models
        (gpdla_batch_absorption_distribution; the definitions are in include/gpdla.h), where ``mean_absorption`` and
        ``var_absorption`` stop at two moments: with abar the broadened profile clamped to [0, 1],

        ``prob_below [T, total]``: the posterior probability that abar <= ``thresholds[j]`` (1 to 4 thresholds strictly inside
        (0, 1)) -- what a forest mask is cut from (:func:`forest_mask`);
        ``absorption_min``, ``absorption_max``: the extremes of abar over the samples and models of positive weight;
        ``quantiles [Q, total]`` (``levels``: 1 to 8 strictly inside (0, 1)): the credible bands of the absorber profile, read off
        a histogram of ``bins`` (8 .. 256) equal bins -- exact where the pixel is unabsorbed (1) or saturated (0), within one
        bin width elsewhere;
        ``histogram [bins, total]`` (``histogram=True``): the masses of the bins themselves.

        ``selection``, ``weights``, ``components``, ``model_weights``, ``meanflux``: as :meth:`marginal_continuum`
        (``weights="refined"`` included: the DLA component on the refined table; ``weights=None`` with ``components=("null",)``
        is the unabsorbed answer).  A call without ``levels`` and ``histogram`` runs the kernel without bins.
        Returns those with ``offsets [nsel + 1]`` and ``status [nsel]`` in the CSR layout of :meth:`model_spectra`."""
        rq = _lib.AbsorptionDistributionRequest()
        sel, keep = self._mixture_request(rq, selection, weights, components, model_weights, meanflux)
        shapes = self._distribution_request(rq, thresholds, bins, levels, histogram, keep)
        out = self._grid_product("absorption_distribution", rq, sel, _lib.AbsorptionDistribution(), shapes)
        del keep
        return out

    def absorption_distribution_multi(self, selection=None, tables="resident", model_weights=None, thresholds=(0.8,),
                                      bins: int = 64, levels=None, histogram: bool = False, meanflux: bool | None = None) -> dict:
        """:meth:`absorption_distribution` over ALL models of a multi-DLA run (gpdla_batch_absorption_distribution_multi): the
        components, ``tables``, ``model_weights`` and ``model_flags`` of :meth:`marginal_continuum_multi` -- sample i of model
        DLA(n) absorbs with the product of the n profiles of its slots."""
        rq = _lib.AbsorptionDistributionMultiRequest()
        sel, _md, keep = self._mixture_multi_request(rq, selection, tables, model_weights, meanflux)
        shapes = self._distribution_request(rq, thresholds, bins, levels, histogram, keep)
        out = self._grid_product_multi("absorption_distribution_multi", rq, sel, _lib.AbsorptionDistributionMulti(), shapes)
        del keep
        return out

    # ---- refined posteriors ----

    def _selection(self, selection):
        return np.arange(self.num_quasars, dtype=np.int64) if selection is None else \
            np.ascontiguousarray(selection, dtype=np.int64).reshape(-1)

    def refine(self, selection=None, levels: int = 2, delta: float = 12.5, pad: float = 2.0, prior=None,
               with_samples: bool = True, download: bool = True) -> dict | None:
        """Zoom boxes of (z_DLA, log N_HI) around the posterior mass of the selected quasars, re-swept on
        the context's refine points (gpdla_batch_refine, after :meth:`process`; the definitions are in
        include/gpdla.h).  ``prior``: a :class:`samples.NhiPrior` (None: uniform over the range of the log N
        samples).  Returns ``selection``, ``boxes`` [n, levels, 4] as (z_lo, z_hi, n_lo, n_hi),
        ``log_likelihoods_dla_refined``, ``log_posteriors_dla_refined``, ``MAP_z_dlas_refined``,
        ``MAP_log_nhis_refined``, ``MAP_inds_refined`` (1-based), ``status`` and, ``with_samples``, the last
        level's ``sample_log_likelihoods_refined`` and ``sample_log_posteriors_refined`` [n, S'].  The
        batch's own results are not touched.  ``download=False``: only launch (asynchronous on the context's
        stream) and return None; :meth:`download_refined` fetches the results."""
        from . import refine as _refine
        if self.ctx.refine_points is None:
            self.ctx.set_refine_points()
        sel = self._selection(selection)
        rq = _refine.request(levels, delta, pad)
        ps = C.byref(prior._s) if prior is not None else None
        _lib.check(self.ctx.lib.gpdla_batch_refine(self.ctx._h, self._h, sel.ctypes.data_as(_i64p),
                                                   sel.size, C.byref(rq), ps))
        self._refined = (int(levels), int(self.ctx.refine_points[0].size))
        return self.download_refined(sel, None, with_samples) if download else None

    def download_refined(self, selection=None, levels: int | None = None, with_samples=True, out: dict | None = None,
                         at: int = 0) -> dict:
        """The resident results of the last :meth:`refine` for quasars of its selection
        (gpdla_batch_download_refined).  The arrays are sized by what that call was made with -- its levels
        and the point set of that time, which the batch remembers; ``levels``, if given, must agree.  The
        library checks the sizes again and refuses a mismatch.  ``with_samples``: True (both sample tables),
        False, or the names of the tables wanted -- a table not asked for is not copied off the device.
        ``out`` / ``at``: write the rows into rows ``at .. at + n`` of arrays made by
        :func:`refine.empty_results` (a pipeline's one set of output arrays) instead of allocating; keys
        ``out`` does not hold are not downloaded."""
        from . import refine as _refine
        if self._refined is None:
            raise _lib.GpdlaError(_lib.ERR_INVALID_ARGUMENT, "the batch has not been refined")
        last_levels, num_points = self._refined
        if levels is not None and int(levels) != last_levels:
            raise ValueError(f"levels = {levels}, but the batch was refined with {last_levels} levels")
        sel = self._selection(selection)
        fields = {name for name, _ in _lib.RefinedResults._fields_}
        if out is None:
            out, at = _refine.empty_results(sel.size, last_levels, num_points, with_samples), 0
            views = out
        else:
            views = {name: a[at:at + sel.size] for name, a in out.items() if name in fields}
            if views["boxes"].shape[1:] != (last_levels, 4) or any(
                    views[k].shape[1] != num_points for k in _refine.TABLES if k in views):
                raise ValueError("the output arrays were not made for this refine's levels and points")
        r = _lib.RefinedResults()
        r.levels, r.num_points = last_levels, num_points
        for name, view in views.items():
            if name in fields:
                assert view.flags.c_contiguous and view.shape[0] == sel.size
                setattr(r, name, view.ctypes.data_as(_i32p if name == "status" else _dp))
        _lib.check(self.ctx.lib.gpdla_batch_download_refined(self.ctx._h, self._h, sel.ctypes.data_as(_i64p),
                                                             sel.size, C.byref(r)))
        if views is out:
            out["selection"] = sel
        return out

    def refined_posteriors(self, selection=None) -> dict:
        """The model posteriors of the selected quasars with the refined evidence in the place of the first
        pass's (gpdla_batch_refined_posteriors, after :meth:`refine`):
        ``model_posteriors_refined`` [n, 2], ``p_no_dlas_refined``, ``p_dlas_refined`` and ``refined`` (1: from
        the refined evidence; 0: the quasar was not refined or is unusable, and the three hold the first
        pass's numbers)."""
        from . import refine as _refine
        sel = self._selection(selection)
        out = _refine.empty_posteriors(sel.size)
        r = _lib.RefinedPosteriors(*[out[name].ctypes.data_as(ct) for name, ct in _lib.RefinedPosteriors._fields_])
        _lib.check(self.ctx.lib.gpdla_batch_refined_posteriors(self.ctx._h, self._h, sel.ctypes.data_as(_i64p),
                                                               sel.size, C.byref(r)))
        return out

    # ---- parameter summaries ----

    def parameter_summaries(self, selection=None, multi: bool = False, sub_dla: bool = False, probabilities=None,
                            thresholds=None, num_models: int | None = None, refined: bool = False) -> dict:
        """Credible intervals and moments of the absorber parameters of the selected quasars from the
        batch's RESIDENT sample tables (gpdla_batch_parameter_summaries) after :meth:`process`
        (``multi=False``) or :meth:`process_multi` (``multi=True``: all ``max_dlas`` models, slots
        gathered through the resident ``base_sample_inds``; ``sub_dla``: the sub-DLA table with the LLS
        column densities, one model).  No second sweep and no download of the table.  Returns what
        :func:`posteriors.parameter_summaries` returns, plus ``selection``.  ``refined``: the summaries of
        the last level of :meth:`refine` instead -- the resident lambda table as weights over the points of
        each quasar's own box (gpdla_batch_refined_summaries), in the same units."""
        from . import posteriors
        p, t = posteriors.check_request(posteriors.DEFAULT_PROBABILITIES if probabilities is None else probabilities,
                                        posteriors.DEFAULT_THRESHOLDS if thresholds is None else thresholds)
        sel = self._selection(selection)
        if refined:
            if multi or sub_dla or num_models not in (None, 1):
                raise ValueError("refined=True: the refined table holds one single-DLA model (no multi, sub_dla or num_models)")
            out, ps = posteriors._outputs(sel.size, 1, len(p), len(t))
            rq = posteriors._request(1, p, t)
            _lib.check(self.ctx.lib.gpdla_batch_refined_summaries(
                self.ctx._h, self._h, sel.ctypes.data_as(_i64p), sel.size, C.byref(rq), C.byref(ps)))
            last = self.download_refined(sel, None, with_samples=False)["boxes"][:, -1]   # the z range the rows were summarised on
            out = posteriors.finish(out, last[:, 0], last[:, 1], self.ctx._log_nhi_scale[0], p, t)
            out["selection"] = sel
            return out
        md = int(num_models) if num_models is not None else (self.max_dlas if (multi and not sub_dla) else 1)
        out, ps = posteriors._outputs(sel.size, md, len(p), len(t))
        rq = posteriors._request(md, p, t)
        _lib.check(self.ctx.lib.gpdla_batch_parameter_summaries(
            self.ctx._h, self._h, int(bool(multi)), int(bool(sub_dla)), sel.ctypes.data_as(_i64p),
            sel.size, C.byref(rq), C.byref(ps)))
        res = self.download_multi(with_samples=False) if self.max_dlas else self.download(with_samples=False)
        z_min, z_max = res["min_z_dlas"][sel], res["max_z_dlas"][sel]
        out = posteriors.finish(out, z_min, z_max, self.ctx._log_nhi_scale[int(bool(sub_dla))], p, t)
        out["selection"] = sel
        return out

    # ---- posterior maps ----

    def posterior_maps(self, selection=None, multi: bool = False, sub_dla: bool = False, refined: bool = False, grid=None,
                       shape=(32, 32), levels=None, mix: bool = True, with_maps: bool = True, num_models: int | None = None,
                       model_weights=None) -> dict:
        """Posterior maps of (z_DLA, log N_HI) of the selected quasars from the batch's RESIDENT tables
        (gpdla_batch_posterior_maps; ``multi`` / ``sub_dla`` as :meth:`parameter_summaries` takes them), or,
        ``refined``, from the last level of :meth:`refine` (gpdla_batch_refined_posterior_maps).  ``grid``:
        (gz_lo, gz_hi, gn_lo, gn_hi) for all quasars or [n, 4]; None: the search range and the log N range of
        the table in use (``refined``: the quasar's last box).  ``mix``: the absorber intensity, weighted by
        ``model_weights`` [n, models] or, None, by the resident model posteriors of DLA(1 ..) (p_lls for the
        sub-DLA table, p_dla for a single-DLA batch, refined or not).  ``with_maps`` False: no per-cell
        array of a slot leaves the device.  Returns what :func:`posteriors.posterior_maps` returns, plus
        ``selection``."""
        from . import posteriors
        shape, lv = posteriors.check_maps_request(shape, posteriors.DEFAULT_LEVELS if levels is None else levels)
        sel = self._selection(selection)
        n = sel.size
        if refined and (multi or sub_dla or num_models not in (None, 1)):
            raise ValueError("refined=True: the refined table holds one single-DLA model (no multi, sub_dla or num_models)")
        md = 1 if refined else (int(num_models) if num_models is not None else (self.max_dlas if (multi and not sub_dla) else 1))
        # The default grid is made here and handed over, so that the grid returned is the grid used: the search
        # range as the downloads report it (NaN for a quasar that was not processed: a bad grid).
        if n and (sel.min() < 0 or sel.max() >= self.num_quasars):
            raise ValueError(f"selection outside the batch of {self.num_quasars} quasars")
        if grid is not None:
            g = posteriors._grid_rows(grid, n)
        elif refined:
            g = np.ascontiguousarray(self.download_refined(sel, None, with_samples=False)["boxes"][:, -1]) if n else np.zeros((0, 4))
        else:
            res = self.download_multi(with_samples=False) if self.max_dlas else self.download(with_samples=False)
            lo, hi = self.ctx._log_nhi_range[int(bool(sub_dla))]
            g = np.ascontiguousarray(np.stack([res["min_z_dlas"][sel], res["max_z_dlas"][sel], np.full(n, lo), np.full(n, hi)], axis=1))
        keep = posteriors._grid_columns(g)                          # (alive until the call returns)
        cols = [_lib.ptr(c) for c in keep]
        w = None if model_weights is None else posteriors._weights_rows(model_weights, n, md)
        use_mix = bool(mix) or w is not None
        out, pm = posteriors.maps_outputs(n, md, shape, len(lv), use_mix, with_maps)
        rq = posteriors.maps_request(md, shape, lv, mix=use_mix)
        wp = _lib.ptr(w) if w is not None else None
        if refined:
            _lib.check(self.ctx.lib.gpdla_batch_refined_posterior_maps(
                self.ctx._h, self._h, sel.ctypes.data_as(_i64p), n, *cols, wp, C.byref(rq), C.byref(pm)))
        else:
            _lib.check(self.ctx.lib.gpdla_batch_posterior_maps(
                self.ctx._h, self._h, int(bool(multi)), int(bool(sub_dla)), sel.ctypes.data_as(_i64p), n, *cols, wp,
                C.byref(rq), C.byref(pm)))
        out = posteriors.finish_maps(out, g, shape, lv)
        out["selection"] = sel
        return out

    # ---- mock spectra ----

    MOCK_COMPONENTS = ("absorption", "continuum", "sigma", "latents")

    def draw_mocks(self, absorbers=None, seed: int | None = None, meanflux: bool | None = None,
                   write_resident: bool = True, components=()) -> dict:
        """One draw per quasar from the model the sweeps evaluate (gpdla_batch_draw_mocks):
        ``flux = a (mu + M z) + sqrt(a^2 omega2 + nu) eps`` on the kept pixels of each quasar's
        unmasked-range grid, with the prepared rows of this batch, its stored noise variance and the
        instrument-broadened absorption ``a`` of the listed absorbers.

        ``absorbers``: ``(offsets [nq + 1], z_dlas, log_nhis)`` in CSR form over the quasars of the batch
        (what :func:`gp_dla_detection_amd.mocks.draw_truth` returns), at most 8 each; None: none.
        ``seed``: 64-bit seed of the Philox streams (default: the context's ``rng_seed``); the key also
        carries ``first_quasar_index + q``, so a quasar's draw does not depend on its batch.
        ``meanflux``: rows of the mean-flux model (default: on for a multi-DLA batch).
        ``write_resident``: the batch's resident flux becomes the draw, and the next :meth:`process` /
        :meth:`process_multi` sweeps it without another upload.
        ``components``: any of ``"absorption"``, ``"continuum"``, ``"sigma"`` (flat, per grid pixel, with
        ``grid_offsets``) and ``"latents"`` (``[nq, k]``).
        Returns ``flux`` (flat, upload layout: masked pixels of the grid are NaN, stored pixels outside
        the modelled range keep the uploaded flux), ``status`` and the requested components."""
        lib = self.ctx.lib
        nq = self.num_quasars
        unknown = set(components) - set(self.MOCK_COMPONENTS)
        if unknown:
            raise ValueError(f"components: any of {self.MOCK_COMPONENTS}, got {sorted(unknown)}")
        rq = _lib.MockRequest()
        rq.seed = int(getattr(self.ctx.params, "rng_seed", 0x9E3779B97F4A7C15) if seed is None else seed) & (2 ** 64 - 1)
        keep = []
        _absorber_fields(rq, absorbers, nq, keep, "quasars")
        rq.meanflux = int(bool(self.max_dlas) if meanflux is None else bool(meanflux))
        rq.write_resident = int(bool(write_resident))
        _lib.check(lib.gpdla_mock_validate(C.byref(rq), nq))  # refused requests never reach the device
        grid = set(components) & {"absorption", "continuum", "sigma"}
        total = int(self.unmasked_counts().sum()) if grid else 0
        rq.capacity_stored, rq.capacity_grid = self.num_pixels, total
        out = {"flux": np.empty(self.num_pixels), "status": np.zeros(nq, dtype=np.int32),
               "grid_offsets": np.zeros(nq + 1, dtype=np.int64)}
        ms = _lib.MockSpectra()
        ms.flux = out["flux"].ctypes.data_as(_dp)
        ms.grid_offsets = out["grid_offsets"].ctypes.data_as(_i64p)
        ms.status = out["status"].ctypes.data_as(_i32p)
        for name in grid:
            out[name] = np.empty(total)
            setattr(ms, name, out[name].ctypes.data_as(_dp))
        if "latents" in components:
            out["latents"] = np.empty((nq, self.ctx.k))
            ms.latents = out["latents"].ctypes.data_as(_dp)
        _lib.check(lib.gpdla_batch_draw_mocks(self.ctx._h, self._h, C.byref(rq), C.byref(ms)))
        return out

    def summary_tensor(self):
        """The per-quasar summary table as a zero-copy torch tensor on this GPU: [nq, 15] for a
        single-DLA batch, [nq, GPDLA_SUMMARY_COLS_MULTI(max_dlas)] (78 for max_dlas = 4) for a
        multi-DLA batch.  This is the row a multi-GPU run all-gathers."""
        import torch
        p, n = C.c_void_p(), C.c_int64()
        if self.max_dlas:
            cols = C.c_int32()
            _lib.check(self.ctx.lib.gpdla_batch_summary_multi_device_ptr(self._h, C.byref(p), C.byref(n),
                                                                         C.byref(cols)))
            ncol = cols.value
        else:
            _lib.check(self.ctx.lib.gpdla_batch_summary_device_ptr(self._h, C.byref(p), C.byref(n)))
            ncol = _lib.SUMMARY_COLS
        return torch.as_tensor(_DeviceArray(p.value, (n.value, ncol), self),
                               device=f"cuda:{self.ctx.device}")

    # ---- multi-DLA batch (process_qsos_multiple_dlas_meanflux.m:141-495) ----

    def process_multi(self, base_sample_inds=None):
        """Launch the multi-DLA driver for every quasar of the batch.  ``base_sample_inds``:
        optional uint32 [nq, max_dlas-1, S], 1-based (0 = never drawn); omitted, the resampling
        of :467-472 is drawn on the GPU."""
        nq, md, S = self.num_quasars, self.max_dlas, self.num_samples
        base_ptr = None
        if base_sample_inds is not None:
            base = np.ascontiguousarray(base_sample_inds, dtype=np.uint32)
            if base.shape != (nq, md - 1, S):
                raise _lib.GpdlaError(-1, f"base_sample_inds must be [nq, max_dlas-1, S], got {base.shape}")
            base_ptr = base.ctypes.data_as(C.POINTER(C.c_uint32))
        _lib.check(self.ctx.lib.gpdla_batch_process_multi(self.ctx._h, self._h, base_ptr))
        self._multi_processed = True

    @staticmethod
    def empty_results_multi(nq: int, md: int, S: int, with_samples: bool = True) -> dict:
        """Host arrays for the variables the multi-DLA script saves (:498-510), for ``nq`` quasars."""
        out = {
            "min_z_dlas": np.full(nq, np.nan), "max_z_dlas": np.full(nq, np.nan),
            "log_likelihoods_no_dla": np.full(nq, np.nan),
            "log_likelihoods_dla": np.full((nq, md), np.nan), "log_likelihoods_lls": np.full(nq, np.nan),
            "log_posteriors_no_dla": np.full(nq, np.nan), "log_posteriors_lls": np.full(nq, np.nan),
            "log_posteriors_dla": np.full((nq, md), np.nan),
            "model_posteriors": np.full((nq, 2 + md), np.nan),
            "p_no_dlas": np.full(nq, np.nan), "p_lls": np.full(nq, np.nan), "p_dlas": np.full(nq, np.nan),
            "MAP_z_dlas": np.full((nq, md, md), np.nan), "MAP_log_nhis": np.full((nq, md, md), np.nan),
            "MAP_inds": np.full((nq, md, md), np.nan),
            "status": np.zeros(nq, dtype=np.int32),
            "log_priors_no_dla": np.full(nq, np.nan), "log_priors_lls": np.full(nq, np.nan),
            "log_priors_dla": np.full((nq, md), np.nan), "all_exceptions": np.full(nq, np.nan),
        }
        if with_samples:
            out["sample_log_likelihoods_dla"] = np.empty((nq, md, S))
            out["sample_log_likelihoods_lls"] = np.empty((nq, S))
            out["base_sample_inds"] = np.zeros((nq, md - 1, S), dtype=np.uint32)
        return out

    def download_multi(self, with_samples: bool = True, out: dict | None = None, at: int = 0) -> dict:
        """Results under the variable names the multi-DLA script saves (:498-510); 3-D arrays are
        ``sample_log_likelihoods_dla [nq, max_dlas, S]`` and ``MAP_* [nq, model, slot]``.
        ``out`` / ``at``: as in :meth:`download`."""
        nq, md, S = self.num_quasars, self.max_dlas, self.num_samples
        if out is None:
            out, at = self.empty_results_multi(nq, md, S, with_samples), 0
        r = _lib.ResultsMulti()
        for name, _ in _lib.ResultsMulti._fields_:
            if name in out and out[name].size:
                ct = {"status": C.c_int32, "base_sample_inds": C.c_uint32}.get(name, C.c_double)
                view = out[name][at:at + nq]
                assert view.flags.c_contiguous and view.shape[0] == nq
                setattr(r, name, view.ctypes.data_as(C.POINTER(ct)))
        _lib.check(self.ctx.lib.gpdla_batch_download_multi(self.ctx._h, self._h, C.byref(r)))
        out["log_priors_no_dla"][at:at + nq] = self.log_priors_no_dla
        out["log_priors_lls"][at:at + nq] = self.log_priors_lls
        out["log_priors_dla"][at:at + nq] = self.log_priors_dla
        out["all_exceptions"][at:at + nq] = np.where(out["status"][at:at + nq] == 1, 1.0, np.nan)  # multi :139, :232
        return out

    def samples_multi_tensors(self):
        """(sample_log_likelihoods_dla [nq, max_dlas, S], sample_log_likelihoods_lls [nq, S]) of a
        multi-DLA batch as zero-copy torch tensors on this GPU."""
        import torch
        a, b = C.c_void_p(), C.c_void_p()
        _lib.check(self.ctx.lib.gpdla_batch_samples_multi_device_ptr(self._h, C.byref(a), C.byref(b), None))
        nq, md, S = self.num_quasars, self.max_dlas, self.num_samples
        dev = f"cuda:{self.ctx.device}"
        return (torch.as_tensor(_DeviceArray(a.value, (nq, md, S), self), device=dev),
                torch.as_tensor(_DeviceArray(b.value, (nq, S), self), device=dev))

    def samples_tensor(self):
        """sample_log_likelihoods_dla [nq, S] as a zero-copy torch tensor on this GPU."""
        import torch
        p, n, s = C.c_void_p(), C.c_int64(), C.c_int64()
        _lib.check(self.ctx.lib.gpdla_batch_samples_device_ptr(self._h, C.byref(p), C.byref(n),
                                                               C.byref(s)))
        return torch.as_tensor(_DeviceArray(p.value, (n.value, s.value), self),
                               device=f"cuda:{self.ctx.device}")

    def close(self):
        if self._h:
            self.ctx.lib.gpdla_batch_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ----------------------------------------------------------------------------------------------
# the script surface
# ----------------------------------------------------------------------------------------------

def record_bytes_per_quasar(num_pixels: int, k: int, slim: bool = True) -> int:
    """Bytes of K-step records (one per 4 pixels) a quasar of ``num_pixels`` stored pixels needs in
    the record pool: 896 B per step for k <= 20 (k_sweep_slim / k_sweep_multi_slim: the M rows, pixel
    rows and wavelengths), 1536 B for 20 < k <= 40 (k_sweep_split_slim: the M rows);
    ``slim=False``: the pre-expanded records of k_sweep / k_sweep_split -- 7680 B and 29 696 B --
    used by the fp32 study and libgpdla_legacy.so's ``GPDLA_EXPANDED_RECORDS=1`` only (every fp64 line count has slim records).  The
    pool of the single-DLA sweep is bounded by ``Parameters.record_pool_bytes`` whatever the batch
    size (the library sweeps group by group)."""
    per_step = ((896 if slim else 7680) if k <= 20 else (1536 if slim else 29696))
    return int((num_pixels / 4 + 2) * per_step)


def resident_bytes_per_quasar(num_pixels: int, k: int, num_samples: int, multi_models: int = 0) -> int:
    """HBM a quasar occupies in a resident batch apart from the record pool: its spectrum, the
    interpolated rows (k + 4 doubles per pixel), the padded wavelengths and its result tables."""
    rows = (num_pixels + 8) * (k + 4 + 1 + 3.2) * 8
    return int(rows + 8 * num_samples * max(1, 2 * multi_models))


def default_batch_size(num_quasars: int, longest: int, k: int, num_samples: int, slots: int,
                       budget_bytes: float = 96 * 2**30, multi_models: int = 0) -> int:
    """Quasars per batch of the host pipeline (gpdla_default_batch_quasars, the rule the one-shot C
    entries apply to themselves): small enough that ``slots`` batches fit ``budget_bytes`` of HBM next
    to the record pool and that a run has ~8 batches to overlap (the first upload and the last
    download are the only copies not hidden behind a sweep), at least 128 so that a launch fills the
    256 CUs many times over."""
    return int(_lib.load().gpdla_default_batch_quasars(int(num_quasars), int(longest), int(k), int(num_samples),
                                                       int(slots), int(budget_bytes), int(multi_models)))


def batch_blocks(num_quasars: int, per_batch: int) -> list:
    """[lo, hi) blocks of a pipelined run.  (Equal blocks: a short first block would start the GPU
    2 ms earlier, but the slot it leaves behind has to grow when it is re-filled, and a hipFree
    waits for the sweeps in flight.)"""
    per_batch = max(1, int(per_batch))
    return [(lo, min(lo + per_batch, num_quasars)) for lo in range(0, num_quasars, per_batch)]


def prefault(*arrays):
    """Touch every page of freshly allocated output arrays (one write per 4 KiB).  Done on the
    download thread while the first batch is swept: a device-to-host copy into untouched pageable
    memory runs at page-fault speed (4 GB/s measured; 10+ once the pages exist)."""
    for a in arrays:
        flat = a.reshape(-1)
        flat[::max(1, 4096 // a.itemsize)] = 0


def run_pipeline(ctx: "Context", num_blocks: int, inputs, process, download, slots: int = 3, warm=None):
    """The host loop of process_qsos.m:88 as a three-stage pipeline over HBM-resident batches:
    while batch i is swept, batch i+1 is prepared and uploaded by one thread and batch i-1
    downloaded by another (the library's copy streams run beside the compute stream; ctypes
    releases the GIL inside the calls).  ``inputs(i)`` returns the arguments of ``Context.upload``
    for block i; ``process(i, batch)`` launches its sweep (main thread, in order);
    ``download(i, batch)`` fetches its results.  ``slots`` batches exist at a time and are
    re-filled in place, so the steady state allocates nothing.  ``warm``: a callable run once on the
    download thread before the first download (e.g. :func:`prefault` of the output arrays)."""
    from concurrent.futures import ThreadPoolExecutor
    if num_blocks <= 0:
        return
    slots = max(1, min(slots, num_blocks))
    batches = [None] * slots
    done = [None] * num_blocks
    up_pool, down_pool = ThreadPoolExecutor(1), ThreadPoolExecutor(1)

    def upload(i):
        slot = i % slots
        if i >= slots:
            done[i - slots].result()  # the slot's previous results are on the host
        args = inputs(i)
        if batches[slot] is None:
            batches[slot] = ctx.upload(*args)
        else:
            batches[slot].reload(*args)
        return batches[slot]

    try:
        nxt = up_pool.submit(upload, 0)
        warmed = down_pool.submit(warm) if warm is not None else None
        for i in range(num_blocks):
            batch = nxt.result()
            # upload(i + 1) waits for done[i + 1 - slots]: with one slot that is THIS block's
            # download, which does not exist before the sweep is launched
            if slots > 1 and i + 1 < num_blocks:
                nxt = up_pool.submit(upload, i + 1)
            process(i, batch)
            done[i] = down_pool.submit(download, i, batch)
            if slots == 1 and i + 1 < num_blocks:
                nxt = up_pool.submit(upload, i + 1)
        for f in done:
            f.result()
        if warmed is not None:
            warmed.result()
    finally:
        up_pool.shutdown(wait=True)
        down_pool.shutdown(wait=True)
        for b in batches:
            if b is not None:
                b.close()


def _model_struct(model: dict, keep: list) -> "_lib.Model":
    rw, rwp = _f64(model["rest_wavelengths"])
    mu, mup = _f64(model["mu"])
    Mf = np.asfortranarray(model["M"], dtype=np.float64)
    lo, lop = _f64(model["log_omega"])
    keep += [rw, mu, Mf, lo]
    return _lib.Model(rw.size, Mf.shape[1], rwp, mup, Mf.ctypes.data_as(_dp), lop,
                      float(model["log_c_0"]), float(model["log_tau_0"]), float(model["log_beta"]))


def _samples_struct(samples: dict, keep: list) -> "_lib.Samples":
    off, offp = _f64(samples["offset_samples"])
    nhi, nhip = _f64(samples["nhi_samples"])
    keep += [off, nhi]
    lnp = llp = None
    if samples.get("log_nhi_samples") is not None:
        a, lnp = _f64(samples["log_nhi_samples"])
        keep.append(a)
    if samples.get("lls_nhi_samples") is not None:
        a, llp = _f64(samples["lls_nhi_samples"])
        keep.append(a)
    return _lib.Samples(off.size, offp, lnp, nhip, llp)


def _spectra_struct(csr: dict, lp_no, lp_dla, lp_lls, keep: list) -> "_lib.Spectra":
    def ptr(a, dt, ct):
        a = np.ascontiguousarray(a, dtype=dt)
        keep.append(a)
        return a.ctypes.data_as(C.POINTER(ct))
    return _lib.Spectra(
        csr["z_qsos"].size, ptr(csr["offsets"], np.int64, C.c_int64),
        ptr(csr["wavelengths"], np.float64, C.c_double), ptr(csr["flux"], np.float64, C.c_double),
        ptr(csr["noise_variance"], np.float64, C.c_double), ptr(csr["pixel_mask"], np.uint8, C.c_uint8),
        ptr(csr["z_qsos"], np.float64, C.c_double), ptr(lp_no, np.float64, C.c_double),
        ptr(lp_dla, np.float64, C.c_double), None if lp_lls is None else ptr(lp_lls, np.float64, C.c_double))


_addressof, _char_from_buffer = C.addressof, C.c_char.from_buffer


def _data_address(a: np.ndarray) -> int:
    """Address of an array's first byte.  Through the buffer protocol where that works (a writable,
    non-empty array: 0.3 us), else through ``__array_interface__`` (1 us: a dict is built per call) --
    a list of 2048 quasars is 8192 arrays."""
    try:
        return _addressof(_char_from_buffer(a))
    except (TypeError, ValueError, BufferError):
        return a.__array_interface__["data"][0]


def _cells_struct(spectra, lp_no, lp_dla, lp_lls, keep: list) -> "_lib.SpectraCells":
    """gpdla_spectra_cells over a list of per-quasar dicts: pointers to the arrays as they are (an
    array that is not contiguous float64 -- uint8 / bool for the mask -- is converted, that one only).
    Column by column, in comprehensions: the per-quasar Python work is what a 2048-quasar call pays
    before the library starts (5 us per quasar as one loop with ``__array_interface__``, 1.5 us so)."""
    n = len(spectra)
    f64, u8, b1, nd = np.dtype(np.float64), np.dtype(np.uint8), np.dtype(np.bool_), np.ndarray
    ptrs = np.empty((4, n), dtype=np.uintp)
    sizes = []
    for j, key in enumerate(("wavelengths", "flux", "noise_variance", "pixel_mask")):
        col = [s[key] for s in spectra]
        if j < 3:
            fix = [i for i, a in enumerate(col) if not (type(a) is nd and a.dtype == f64 and a.flags.c_contiguous)]
            for i in fix:
                col[i] = np.ascontiguousarray(col[i], dtype=np.float64)
        else:
            fix = [i for i, a in enumerate(col)
                   if not (type(a) is nd and (a.dtype == u8 or a.dtype == b1) and a.flags.c_contiguous)]
            for i in fix:
                col[i] = np.ascontiguousarray(col[i], dtype=np.uint8)
        keep.append(col)
        ptrs[j] = [_data_address(a) for a in col]
        sizes.append(np.array([a.size for a in col], dtype=np.int64))
    npix = sizes[0]
    same = (sizes[1] == npix) & (sizes[2] == npix) & (sizes[3] == npix)
    if not same.all():
        raise _lib.GpdlaError(-1, f"quasar {int(np.flatnonzero(~same)[0])}: wavelengths, flux, noise_variance and pixel_mask differ in length")
    z = np.array([s["z_qso"] for s in spectra], dtype=np.float64)
    keep += [ptrs, npix, z]

    def dptr(a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        keep.append(a)
        return a.ctypes.data_as(_dp)
    return _lib.SpectraCells(n, npix.ctypes.data_as(_i64p), ptrs[0].ctypes.data, ptrs[1].ctypes.data,
                             ptrs[2].ctypes.data, ptrs[3].ctypes.data, z.ctypes.data_as(_dp), dptr(lp_no), dptr(lp_dla),
                             None if lp_lls is None else dptr(lp_lls))


def _result_struct(struct_type, out: dict):
    r = struct_type()
    for name, _ in struct_type._fields_:
        if name in out and out[name].size:
            ct = {"status": C.c_int32, "base_sample_inds": C.c_uint32}.get(name, C.c_double)
            assert out[name].flags.c_contiguous
            setattr(r, name, out[name].ctypes.data_as(C.POINTER(ct)))
    return r


def process_qsos(model: dict, samples: dict, spectra, prior_catalog: dict | None = None,
                 params: Parameters | None = None, device: int = 0,
                 log_priors: tuple | None = None, max_quasars_per_batch: int | None = None,
                 pipeline_slots: int = 3, with_samples: bool = True) -> dict:
    """The ``process_qsos`` script (process_qsos.m:4-250) for a list of quasars: a thin caller of
    ``gpdla_process_cells`` (a list: one array per quasar, handed over as it is) or
    ``gpdla_process_batch`` (CSR arrays), the one-shot C entries a MEX gateway binds (INTEGRATION.md
    section 3).

    ``spectra``: list of dicts with ``wavelengths, flux, noise_variance, pixel_mask, z_qso`` (one
    entry of the ``all_*`` cell arrays each, after the ``test_ind`` subset of :56-61), or the CSR
    dict of :func:`spectra_to_csr` (no host copy then).
    ``prior_catalog``: ``{"z_qsos", "dla_ind"}`` of the training release after the Lyman-limit
    filter of :15-25; or pass ``log_priors=(log_priors_no_dla, log_priors_dla)`` directly.
    Quasars are independent, so the library sweeps the list in HBM-resident batches of at most
    ``max_quasars_per_batch`` (default: :func:`default_batch_size`) through ``pipeline_slots`` batch
    slots: uploads and downloads overlap the sweeps.  Results do not depend on the batching.
    Returns the variables the script saves (:236-244)."""
    p = params or Parameters()
    is_csr = isinstance(spectra, dict)
    if not is_csr:
        spectra = list(spectra)
    z_all = spectra["z_qsos"] if is_csr else np.array([float(s_["z_qso"]) for s_ in spectra], dtype=np.float64)
    nq = z_all.size
    if log_priors is None:
        if prior_catalog is None:
            raise ValueError("need prior_catalog or log_priors")
        log_priors = dla_existence_prior(prior_catalog["z_qsos"], prior_catalog["dla_ind"], z_all, p)
    lp_no, lp_dla = (np.ascontiguousarray(x, dtype=np.float64) for x in log_priors)
    S = np.asarray(samples["offset_samples"]).size
    out = Batch.empty_results(nq, S, with_samples) if nq else {}
    if nq:
        lib = _lib.load()
        cfg = _config(p)
        cfg.pipeline_slots = int(pipeline_slots)
        cfg.max_quasars_per_batch = int(max_quasars_per_batch or 0)
        keep = []
        m, s_ = _model_struct(model, keep), _samples_struct(samples, keep)
        r = _result_struct(_lib.Results, out)
        if is_csr:
            sp = _spectra_struct(spectra, lp_no, lp_dla, None, keep)
            rc = lib.gpdla_process_batch(C.byref(m), C.byref(s_), C.byref(sp), C.byref(cfg), C.byref(r), int(device))
        else:  # one array per quasar, as they are: the library flattens block by block beside the sweeps
            sp = _cells_struct(spectra, lp_no, lp_dla, None, keep)
            rc = lib.gpdla_process_cells(C.byref(m), C.byref(s_), C.byref(sp), C.byref(cfg), C.byref(r), int(device))
        _lib.check(rc)
        out["log_priors_no_dla"][:] = lp_no
        out["log_priors_dla"][:] = lp_dla
    out["num_lines"] = p.num_lines
    out["prior_z_qso_increase"] = p.prior_z_qso_increase
    out["max_z_cut"] = p.max_z_cut
    return out


def refine_absorbers(model: dict, samples: dict, spectra, results: dict, p_dla_threshold: float = 0.9, **kw) -> dict:
    """Refine the absorber posteriors of the quasars of ``spectra`` whose ``results["p_dlas"]`` reach
    ``p_dla_threshold``: :func:`refine.refine_absorbers`, which documents the keywords."""
    from . import refine
    return refine.refine_absorbers(model, samples, spectra, results, p_dla_threshold, **kw)


def refine_multi_absorbers(model: dict, samples: dict, spectra, results_multi: dict, **kw) -> dict:
    """Refine the reported absorbers of a multi-DLA run slot by slot, each conditioned on the others of its
    quasar: :func:`conditional.refine_multi_absorbers`; :func:`conditional.refine_conditional`
    documents the keywords."""
    from . import conditional
    return conditional.refine_multi_absorbers(model, samples, spectra, results_multi, **kw)


# ----------------------------------------------------------------------------------------------
# multi-DLA driver
# ----------------------------------------------------------------------------------------------

def dla_existence_prior_multi(prior_z_qsos, prior_dla_ind, z_qsos, Z_lls: float, Z_dla: float,
                              params: MultiParameters | None = None):
    """process_qsos_multiple_dlas_meanflux.m:189-216: priors for exactly 1..max_dlas DLAs
    ((M/N)^k - (M/N)^(k+1)), for a sub-DLA (M/N * Z_lls/Z_dla) and for no absorber.
    Returns (log_priors_no_dla [nq], log_priors_lls [nq], log_priors_dla [nq, max_dlas])."""
    p = params or MultiParameters()
    pz = np.asarray(prior_z_qsos, dtype=np.float64)
    pd = np.asarray(prior_dla_ind, dtype=bool)
    z = np.atleast_1d(np.asarray(z_qsos, dtype=np.float64))
    order = np.argsort(pz, kind="stable")
    cum = np.concatenate([[0], np.cumsum(pd[order])])
    N = np.searchsorted(pz[order], z + p.prior_z_qso_increase, side="left").astype(np.float64)
    M = cum[N.astype(np.int64)].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        pk = (M / N)[:, None] ** np.arange(1, p.max_dlas + 1)[None, :]      # :194
        pk[:, :-1] = pk[:, :-1] - pk[:, 1:]                                  # :197-199
        log_dla = np.log(pk)                                                 # :204
        log_lls = np.log(M) - np.log(N) + np.log(Z_lls) - np.log(Z_dla)      # :208-210
        log_no = np.log(N - M - Z_lls * M / Z_dla) - np.log(N)               # :214-216
    return log_no, log_lls, log_dla


def process_qsos_multiple_dlas_meanflux(model: dict, samples: dict, spectra, log_priors,
                                        params: MultiParameters | None = None,
                                        base_sample_inds=None, device: int = 0,
                                        max_quasars_per_batch: int | None = None,
                                        pipeline_slots: int = 3) -> dict:
    """The multi-DLA driver (multi_dlas/process_qsos_multiple_dlas_meanflux.m:141-510).

    ``samples`` additionally carries ``log_nhi_samples`` and ``lls_nhi_samples``
    (set_lls_parameters.m:59-63).  ``log_priors = (no_dla [nq], lls [nq], dla [nq, max_dlas])`` as
    returned by :func:`dla_existence_prior_multi`.  ``base_sample_inds``: optional uint32
    ``[nq, max_dlas-1, S]``, 1-based (the reference's saved variable, :476, transposed to
    quasar-slowest; rows the reference left zero after its early exit make the samples that
    would consume them NaN); when omitted the resampling of :467-472 is drawn on the GPU
    (Philox4x32-10, ``params.rng_seed``, keyed by ``params.first_quasar_index`` + position, so
    batches and shards of one run draw what the whole run would).  Quasars are independent, so a
    long list is swept in HBM-resident batches of at most ``max_quasars_per_batch``.
    Returns the variables the script saves (:498-510); 3-D arrays are
    ``sample_log_likelihoods_dla [nq, max_dlas, S]`` and ``MAP_* [nq, model, slot]``."""
    p = params or MultiParameters()
    md = p.max_dlas
    S = np.asarray(samples["offset_samples"]).size
    is_csr = isinstance(spectra, dict)
    if not is_csr:
        spectra = list(spectra)
    nq = spectra["z_qsos"].size if is_csr else len(spectra)
    lp_no, lp_lls, lp_dla = (np.ascontiguousarray(x, dtype=np.float64) for x in log_priors)
    lp_dla = lp_dla.reshape(nq, md)
    base_ptr = None
    if base_sample_inds is not None:
        base_sample_inds = np.ascontiguousarray(base_sample_inds, dtype=np.uint32)
        if base_sample_inds.shape != (nq, md - 1, S):
            raise _lib.GpdlaError(-1, "base_sample_inds must be [nq, max_dlas-1, S], got "
                                  f"{base_sample_inds.shape}")
        base_ptr = base_sample_inds.ctypes.data_as(C.POINTER(C.c_uint32))
    out = Batch.empty_results_multi(nq, md, S) if nq else {}
    if nq:
        lib = _lib.load()
        cfg = _config(p)
        cfg.pipeline_slots = int(pipeline_slots)
        cfg.max_quasars_per_batch = int(max_quasars_per_batch or 0)
        keep = []
        m, s_ = _model_struct(model, keep), _samples_struct(samples, keep)
        r = _result_struct(_lib.ResultsMulti, out)
        if is_csr:
            sp = _spectra_struct(spectra, lp_no, lp_dla, lp_lls, keep)
            rc = lib.gpdla_process_batch_multi(C.byref(m), C.byref(s_), C.byref(sp), base_ptr, C.byref(cfg), C.byref(r),
                                               int(device))
        else:
            sp = _cells_struct(spectra, lp_no, lp_dla, lp_lls, keep)
            rc = lib.gpdla_process_cells_multi(C.byref(m), C.byref(s_), C.byref(sp), base_ptr, C.byref(cfg), C.byref(r),
                                               int(device))
        _lib.check(rc)
        out["log_priors_no_dla"][:] = lp_no
        out["log_priors_lls"][:] = lp_lls
        out["log_priors_dla"][:] = lp_dla
        out["all_exceptions"][:] = np.where(out["status"] == 1, 1.0, np.nan)  # multi :139, :232
    return out


# ----------------------------------------------------------------------------------------------
# model spectra
# ----------------------------------------------------------------------------------------------

#: the names of :mod:`grid_fields`, by product and kind
MODEL_SPECTRA_ARRAYS = grid_fields.names("model_spectra")
#: what ``multi_models`` adds: flat per-pixel arrays, and per-model planes [max_dlas, total]
MODEL_SPECTRA_MULTI_ARRAYS = grid_fields.names("model_spectra_multi", "pixel")
MODEL_SPECTRA_MULTI_PLANES = grid_fields.names("model_spectra_multi", "plane")
MARGINAL_CONTINUUM_ARRAYS = grid_fields.names("marginal_continuum", "pixel")
MARGINAL_CONTINUUM_ROWS = grid_fields.names("marginal_continuum", "row", (None, "sample_coefficients"))
PREDICTIVE_FLUX_ARRAYS = grid_fields.names("predictive_flux", "pixel", (None,))
PREDICTIVE_FLUX_RESIDUALS = grid_fields.names("predictive_flux", "pixel", ("residuals",))
PREDICTIVE_FLUX_ROWS = grid_fields.names("predictive_flux", "column")


def renormalised_model_posteriors(results: dict) -> np.ndarray:
    """Model weights ``[nq, 2 + max_dlas]`` as (null, sub-DLA, DLA(1..max_dlas)) from the LOG posteriors of a
    multi-DLA run: a softmax over the finite ``log_posteriors_no_dla``, ``log_posteriors_lls`` and
    ``log_posteriors_dla`` of each quasar, a NaN (or -inf) model getting probability 0.  The reference's early
    exit (multi :460-464) leaves the models it did not reach NaN, and with them the whole ``model_posteriors``
    row (:482-495); this is the row renormalised over the models that were evaluated, for a caller of
    :meth:`Batch.model_spectra_multi` who wants those quasars in the average.  A quasar without any finite
    log posterior keeps a NaN row."""
    null = np.asarray(results["log_posteriors_no_dla"], dtype=np.float64).reshape(-1, 1)
    lp = np.concatenate([null, np.asarray(results["log_posteriors_lls"], dtype=np.float64).reshape(-1, 1),
                         np.asarray(results["log_posteriors_dla"], dtype=np.float64).reshape(null.shape[0], -1)], axis=1)
    finite = np.isfinite(lp)
    mx = np.where(finite, lp, -np.inf).max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        e = np.where(finite, np.exp(np.where(finite, lp, 0.0) - np.where(np.isfinite(mx), mx, 0.0)), 0.0)
        out = e / e.sum(axis=1, keepdims=True)
    out[~finite.any(axis=1)] = np.nan
    return out


def split_cells(flat, offsets) -> list:
    """A flat CSR array as one view per quasar."""
    o = np.asarray(offsets, dtype=np.int64)
    return [flat[o[i]:o[i + 1]] for i in range(o.size - 1)]


def map_absorbers(results: dict, sub_dla: bool = True):
    """The absorbers of each quasar's most probable model, from the saved results, as the CSR triple
    ``(offsets [nq + 1], z_dlas, log_nhis)`` that :meth:`Batch.model_spectra` and
    :func:`dla_model_mean` take.

    Multi-DLA results (``model_posteriors [nq, 1 + sub_dla + max_dlas]``, ``MAP_z_dlas`` /
    ``MAP_log_nhis [nq, model, slot]``) follow the reference's QSOLoader: ``nth = argmax(model_posteriors)
    - 1 - sub_dla`` (qso_loader.py:1695); ``nth >= 0`` selects slots ``0 .. nth`` of model ``nth``
    (:285-301, :1698-1699).  ``sub_dla``: the posteriors carry a sub-DLA column after the null model
    (the multi-DLA driver's always do); a sub-DLA or null winner has no absorbers.  Single-DLA results
    (``model_posteriors [nq, 2]``) give ``MAP_z_dlas`` / ``MAP_log_nhis`` where p_dla wins (:1700-1704).
    A quasar whose posteriors are all NaN has none; a NaN slot of a chosen model is dropped."""
    mp = np.asarray(results["model_posteriors"], dtype=np.float64)
    nq = mp.shape[0]
    map_z = np.asarray(results["MAP_z_dlas"], dtype=np.float64)
    map_n = np.asarray(results["MAP_log_nhis"], dtype=np.float64)
    single = mp.shape[1] == 2 and map_z.ndim == 1
    shift = 1 if single else 1 + int(bool(sub_dla))
    z_out, n_out, offsets = [], [], np.zeros(nq + 1, dtype=np.int64)
    for i in range(nq):
        row = mp[i]
        if not np.isnan(row).all():
            nth = int(np.nanargmax(row)) - shift
            if nth >= 0:
                z, n = (map_z[i:i + 1], map_n[i:i + 1]) if single else (map_z[i, nth, :nth + 1], map_n[i, nth, :nth + 1])
                ok = np.isfinite(z) & np.isfinite(n)
                z_out.append(z[ok])
                n_out.append(n[ok])
        offsets[i + 1] = sum(a.size for a in z_out)
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0)  # noqa: E731
    return offsets, cat(z_out), cat(n_out)


def _take_absorbers(absorbers, idx):
    """The CSR lists of quasars ``idx`` out of a CSR triple."""
    off, z, n = absorbers
    off = np.asarray(off, dtype=np.int64)
    parts = [np.arange(off[i], off[i + 1]) for i in idx]
    take = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
    new = np.zeros(len(parts) + 1, dtype=np.int64)
    np.cumsum([p.size for p in parts], out=new[1:])
    return new, np.asarray(z, dtype=np.float64)[take], np.asarray(n, dtype=np.float64)[take]


def _block_size(max_quasars_per_batch, spectra, idx, model: dict, samples: dict) -> int:
    """Quasars a block of the drivers below: what the caller asked for, or :func:`default_batch_size`."""
    longest = max([np.asarray(spectra[i]["wavelengths"]).size for i in idx], default=1)
    return int(max_quasars_per_batch or default_batch_size(len(idx), longest, np.asarray(model["M"]).shape[1],
                                                           np.asarray(samples["offset_samples"]).size, 1))


def _resident_blocks(model: dict, samples: dict, spectra, idx, params: Parameters, device: int, max_quasars_per_batch, refined=None):
    """Generator over the quasars ``idx`` of ``spectra`` in blocks of :func:`_block_size`, each resident in turn in ONE batch
    of a context of its own (uploaded, then reloaded; placeholder priors, since nothing is swept): yields
    ``(lo, hi, idx[lo:hi], batch)``.  Batch and context are closed when the generator is (``contextlib.closing``
    around the loop makes that every exit path).  An empty ``idx`` yields nothing and loads nothing.  ``refined``: what
    :func:`_refined_options` returns -- the blocks are uploaded with the run's own priors and the context gets the refine
    points, for :func:`_refine_block`."""
    if not len(idx):
        return
    per = _block_size(max_quasars_per_batch, spectra, idx, model, samples)
    multi = isinstance(params, MultiParameters)
    md = params.max_dlas if multi else 0
    ctx = Context(device, params)
    batch = None
    try:
        ctx.set_model(model)
        ctx.set_samples(samples)
        if refined is not None:
            pts = refined["points"]
            if pts is None or np.ndim(pts) == 0:
                ctx.set_refine_points(num=None if pts is None else int(pts))
            else:
                ctx.set_refine_points(*pts)
        for lo, hi in batch_blocks(len(idx), per):
            block = idx[lo:hi]
            n = hi - lo
            args = ([spectra[i] for i in block], np.zeros(n), np.zeros((n, md)) if multi else np.zeros(n),
                    np.zeros(n) if multi else None)
            if refined is not None:
                args = (args[0], refined["log_priors"][0][block], refined["log_priors"][1][block], None)
            if batch is None:
                batch = ctx.upload(*args)
            else:
                batch.reload(*args)
            yield lo, hi, block, batch
    finally:
        if batch is not None:
            batch.close()
        ctx.close()


REFINED_KEYS = ("levels", "delta", "pad", "points", "prior")


def _refined_options(refined, results, params):
    """The ``refined=`` argument of :func:`model_spectra`, :func:`marginal_continuum` and :func:`predictive_flux` checked and
    completed: None, or a dict with ``levels``, ``delta``, ``pad``, ``prior`` (:meth:`Batch.refine`), ``points`` ((u, v), a
    number of default points, or None: as many as there are DLA samples) and the run's ``log_priors``."""
    if refined is None:
        return None
    from . import refine as _refine
    if isinstance(params, MultiParameters):
        raise ValueError("refined: a multi-DLA batch cannot be refined (DESIGN.md 4.18)")
    unknown = set(refined) - set(REFINED_KEYS)
    if unknown:
        raise ValueError(f"refined: unknown keys {sorted(unknown)}; known: {REFINED_KEYS}")
    if results is None or "log_priors_no_dla" not in results or "log_priors_dla" not in results:
        raise ValueError("refined needs results with log_priors_no_dla and log_priors_dla: the selected quasars are processed again")
    opts = dict(levels=_refine.DEFAULT_LEVELS, delta=_refine.DEFAULT_DELTA, pad=_refine.DEFAULT_PAD, points=None, prior=None)
    opts.update({k: v for k, v in refined.items() if v is not None})
    pts = opts["points"]
    _refine.validate(opts["levels"], opts["delta"], opts["pad"], opts["prior"], *((None, None) if pts is None or np.ndim(pts) == 0 else pts))
    opts["log_priors"] = (np.asarray(results["log_priors_no_dla"], dtype=np.float64).reshape(-1),
                          np.asarray(results["log_priors_dla"], dtype=np.float64).reshape(-1))
    return opts


def _refine_block(batch: "Batch", opts: dict) -> dict:
    """The first pass and the refine pass of a resident block (the way :func:`refine_absorbers` works); returns the boxes
    and the refine status of its quasars."""
    batch.process()
    return batch.refine(None, opts["levels"], opts["delta"], opts["pad"], opts["prior"], with_samples=False)


def _posterior_weights(mw: np.ndarray, components) -> np.ndarray:
    """Model posteriors ``[n, 3]`` as (null, sub-DLA, DLA) made into the weights of ``model_weights="posteriors"``: a NaN or
    negative probability weighs 0 (p_dlas is a difference of probabilities and can round to -1e-166), and a quasar whose
    listed posteriors are then all 0 falls back to equal weights over the listed components."""
    mw = np.maximum(np.nan_to_num(mw, nan=0.0), 0.0)
    listed = np.array([c in components for c in ("null", "sub_dla", "dla")])
    empty = ~(mw[:, listed].sum(axis=1) > 0)
    mw[np.ix_(empty, listed)] = 1.0
    return mw


def stitch_blocks(blocks, n: int, per_block, expect, dims: dict, refined: dict | None = None) -> dict:
    """THE block loop of the grid products: ``blocks`` iterates ``(lo, hi, idx, batch)`` over a selection of ``n`` quasars
    (:func:`_resident_blocks`; any iterator will do), ``per_block(batch, idx, lo, hi)`` returns what one or several
    ``Batch`` methods returned for the block (a dict, or a sequence of dicts), and the result is ``offsets [n + 1]`` and
    ``status [n]`` (the OR over the block's dicts) followed by the fields ``expect`` (of :mod:`grid_fields`, which knows each
    one's axis and dtype), stitched in selection order.  ``refined``: what :func:`_refined_options` returns -- each block is
    processed and refined (:func:`_refine_block`) before ``per_block`` sees it, and ``boxes [n, levels, 4]`` and
    ``refine_status [n]`` follow ``status``.  An empty selection returns the same keys with no extent
    (:func:`grid_fields.empty` by ``dims``)."""
    out = {"offsets": np.zeros(n + 1, dtype=np.int64), "status": np.zeros(n, dtype=np.int32)}
    if refined is not None:
        out["boxes"] = np.full((n, int(refined["levels"]), 4), np.nan)
        out["refine_status"] = np.full(n, -1, dtype=np.int32)
    parts = {f.name: [] for f in expect}
    for lo, hi, idx, batch in blocks:
        if refined is not None:
            ref = _refine_block(batch, refined)
            out["boxes"][lo:hi], out["refine_status"][lo:hi] = ref["boxes"], ref["status"]
        results = per_block(batch, idx, lo, hi)
        results = [results] if isinstance(results, dict) else list(results)
        out["offsets"][lo + 1:hi + 1] = out["offsets"][lo] + results[0]["offsets"][1:]
        for res in results:
            out["status"][lo:hi] |= res["status"]
            for name in parts:
                if name in res:
                    parts[name].append(res[name])
    for f in expect:
        out[f.name] = grid_fields.join(f, parts[f.name]) if n else grid_fields.empty(f, dims)
    return out


def _drive(model: dict, samples: dict, spectra, sel, params, device: int, max_quasars_per_batch, per_block, expect,
           refined: dict | None = None, plane_dims: dict | None = None) -> dict:
    """:func:`stitch_blocks` over :func:`_resident_blocks` of the selected quasars, with ``selection`` in front.
    ``plane_dims``: the named leading dimensions of the product's planes (:mod:`grid_fields`)."""
    S = np.asarray(samples["offset_samples"]).size
    if refined is not None and refined["points"] is not None:    # S': the refine points the options name
        S = int(refined["points"]) if np.ndim(refined["points"]) == 0 else np.asarray(refined["points"][0]).size
    dims = dict(k=np.asarray(model["M"]).shape[1], samples=S, max_dlas=int(getattr(params, "max_dlas", 0)), **(plane_dims or {}))
    with closing(_resident_blocks(model, samples, spectra, sel, params, device, max_quasars_per_batch, refined)) as blocks:
        return {"selection": sel, **stitch_blocks(blocks, sel.size, per_block, expect, dims, refined)}


def _selected(spectra, selection) -> np.ndarray:
    return np.arange(len(spectra), dtype=np.int64) if selection is None else np.asarray(selection, dtype=np.int64).reshape(-1)


def _multi_inputs(results, model_weights, multi_rows, posteriors_by_name: bool):
    """``(model_weights [nq, 2 + max_dlas], multi_rows)`` of a ``multi_models`` call: the three tables of ``results`` behind
    ``multi_rows`` when none is given, ``results["model_posteriors"]`` for no weights (and, ``posteriors_by_name``, for
    ``"posteriors"``)."""
    if multi_rows is None:
        if results is None or "base_sample_inds" not in results or np.asarray(results["sample_log_likelihoods_dla"]).ndim != 3:
            raise ValueError("multi_models needs results with base_sample_inds and sample_log_likelihoods_dla [nq, max_dlas, S]")
        multi_rows = lambda idx: {name: np.asarray(results[name])[idx] for name in  # noqa: E731
                                  ("sample_log_likelihoods_dla", "base_sample_inds", "sample_log_likelihoods_lls")}
    if model_weights is None or (posteriors_by_name and isinstance(model_weights, str) and model_weights == "posteriors"):
        if results is None:
            raise ValueError("multi_models needs model_weights or results")
        model_weights = results["model_posteriors"]
    elif posteriors_by_name and isinstance(model_weights, str):
        raise ValueError("model_weights: 'posteriors', an array [nq, 2 + max_dlas] or None")
    return np.asarray(model_weights, dtype=np.float64), multi_rows


def model_spectra(model: dict, samples: dict, spectra, results: dict | None = None,
                  params: Parameters | None = None, selection=None, absorbers="map", sub_dla: bool | None = None,
                  moments_sub_dla: bool = False, products=("map", "moments", "continuum"), sample_rows=None,
                  device: int = 0, max_quasars_per_batch: int | None = None, multi_models: bool = False,
                  model_weights=None, multi_rows=None, refined: dict | None = None) -> dict:
    """Model spectra of the selected quasars of a processed run, batched like :func:`process_qsos`:
    the selected spectra are uploaded block by block and nothing is swept again -- the posterior
    weights come from the saved sample log-likelihoods.

    ``spectra``: the list of per-quasar dicts the run processed; ``results``: what it returned (or
    :func:`io.load_processed_qsos` of its file); ``params``: a :class:`MultiParameters` makes the
    batches multi-DLA ones (mean-flux model).  ``selection``: indices into ``spectra`` (default all).
    ``absorbers``: ``"map"`` (:func:`map_absorbers` of ``results``), a CSR triple over ALL quasars of
    ``spectra``, or None.  ``sub_dla``: whether the posteriors carry a sub-DLA column (default: they do
    for multi-DLA results).  Moments weight the DLA(1) table ``sample_log_likelihoods_dla`` (``[nq, S]``,
    or ``[nq, max_dlas, S]``), or ``sample_log_likelihoods_lls`` with ``moments_sub_dla``;
    ``sample_rows(idx) -> [len(idx), S]`` supplies the rows instead (a file streamed block by block).
    ``multi_models``: also what :meth:`Batch.model_spectra_multi` returns for a multi-DLA run (the moments of
    every model DLA(1 .. max_dlas) and of the sub-DLA model, and their average over the models): ``results``
    must then carry ``base_sample_inds``, the 3-D ``sample_log_likelihoods_dla`` and ``sample_log_likelihoods_lls``
    -- or ``multi_rows(idx)`` returns the dict of those three for quasars ``idx`` -- and ``model_weights``
    ``[nq, 2 + max_dlas]`` over ALL quasars weighs the models (default: ``results["model_posteriors"]``;
    :func:`renormalised_model_posteriors` includes the quasars of the reference's early exit).
    ``refined``: None, or ``dict(levels=, delta=, pad=, points=, prior=)`` (any may be left out): per resident block the
    selected quasars are processed and refined (:meth:`Batch.process`, :meth:`Batch.refine`, the way
    :func:`refine_absorbers` works; ``results`` supplies the priors) and the moments come from the refined table
    (``weights="refined"``: posterior mass outside the last box is ignored).  The result gains ``boxes`` and
    ``refine_status``.  Single-DLA runs only.
    Returns ``selection``, ``offsets``, ``status`` and the flat per-pixel arrays of
    :meth:`Batch.model_spectra`, in selection order; results do not depend on the batching.  An empty selection returns
    every key the same call returns for a non-empty one, each with no extent (:func:`grid_fields.empty`)."""
    p = params or Parameters()
    multi = isinstance(p, MultiParameters)
    refined = _refined_options(refined, results, p)
    if refined is not None and moments_sub_dla:
        raise ValueError("refined: the refined table is the DLA table (no moments_sub_dla)")
    spectra = list(spectra)
    sel = _selected(spectra, selection)
    products = tuple(products)
    if isinstance(absorbers, str):
        if absorbers != "map":
            raise ValueError("absorbers: 'map', a CSR triple or None")
        if results is None:
            raise ValueError("absorbers='map' needs results")
        absorbers = map_absorbers(results, sub_dla=multi if sub_dla is None else sub_dla)
    if "moments" in products and sample_rows is None and refined is None:
        if results is None:
            raise ValueError("moments need results or sample_rows")
        table = np.asarray(results["sample_log_likelihoods_lls" if moments_sub_dla else "sample_log_likelihoods_dla"])
        sample_rows = (lambda idx: table[idx]) if table.ndim == 2 else (lambda idx: table[idx, 0, :])
    expect = grid_fields.requested("model_spectra", products)
    if multi_models:
        model_weights, multi_rows = _multi_inputs(results, model_weights, multi_rows, posteriors_by_name=False)
        expect = grid_fields.requested("multi_models") + expect + grid_fields.requested("model_spectra_multi")

    def per_block(batch, idx, lo, hi):
        if "moments" not in products:
            weights = None
        else:
            weights = "refined" if refined is not None else np.asarray(sample_rows(idx), dtype=np.float64)
        res = [batch.model_spectra(absorbers=None if absorbers is None else _take_absorbers(absorbers, idx),
                                   weights=weights, sub_dla=moments_sub_dla, products=products)]
        if multi_models:
            res.append(batch.model_spectra_multi(tables=multi_rows(idx), model_weights=model_weights[idx]))
        return res
    return _drive(model, samples, spectra, sel, p, device, max_quasars_per_batch, per_block, expect, refined)


def posterior_model_weights(results: dict) -> np.ndarray:
    """``[nq, 3]`` as (p_no_dlas, p_lls or 0, p_dlas) from a results dict or processed file: the model weights
    :func:`marginal_continuum` mixes by with ``model_weights="posteriors"``.  A NaN probability weighs 0, and so does
    a negative one (p_dlas is a difference of probabilities and can round to -1e-166)."""
    p_no = np.asarray(results["p_no_dlas"], dtype=np.float64).reshape(-1)
    p_lls = np.asarray(results["p_lls"], dtype=np.float64).reshape(-1) if "p_lls" in results else np.zeros(p_no.size)
    p_dla = np.asarray(results["p_dlas"], dtype=np.float64).reshape(-1)
    return np.maximum(np.nan_to_num(np.stack([p_no, p_lls, p_dla], axis=1), nan=0.0), 0.0)


def _mixture_inputs(results, components, model_weights, sample_rows):
    """``(components, sampled, model_weights, sample_rows)`` as :func:`marginal_continuum` and
    :func:`predictive_flux` take them: ``"posteriors"`` resolved against ``results``, the tables of ``results``
    behind ``sample_rows`` when none is given."""
    components = tuple(components)
    sampled = [c for c in components if c != "null"]
    if isinstance(model_weights, str):
        if model_weights != "posteriors":
            raise ValueError("model_weights: 'posteriors', an array [nq, 3] or None")
        if results is None:
            raise ValueError("model_weights='posteriors' needs results")
        model_weights = _posterior_weights(posterior_model_weights(results), components)
    elif model_weights is not None:
        model_weights = np.asarray(model_weights, dtype=np.float64)
    if sampled and sample_rows is None:
        if results is None:
            raise ValueError("a sampled component needs results or sample_rows")
        tables = {}
        for name, key in (("dla", "sample_log_likelihoods_dla"), ("sub_dla", "sample_log_likelihoods_lls")):
            if name in sampled:
                t = np.asarray(results[key])
                tables[name] = t if t.ndim == 2 else t[:, 0, :]
        sample_rows = lambda idx, name: tables[name][idx]  # noqa: E731
    return components, sampled, model_weights, sample_rows


def _mixture(product: str, kw: dict, model, samples, spectra, results, params, selection, components, model_weights, sample_rows,
             device, max_quasars_per_batch, multi_models, multi_rows, refined, plane_dims: dict | None = None) -> dict:
    """What :func:`marginal_continuum`, :func:`predictive_flux` and :func:`absorption_distribution` are: ``Batch.<product>(**kw)`` block by block through
    :func:`_drive` -- on the refined table (``refined``), over all models of a multi-DLA run (``multi_models``:
    ``Batch.<product>_multi`` with the switches of ``kw`` that are on) or on the saved tables."""
    p = params or Parameters()
    spectra = list(spectra)
    sel = _selected(spectra, selection)
    refined = _refined_options(refined, results, p)
    on = {name: v for name, v in kw.items() if v}
    # (the multi forms take the switches that are on; an argument that is no switch of a field goes through as given)
    on_multi = {name: v for name, v in kw.items() if v or name in ("thresholds", "bins", "levels")}
    expect = grid_fields.requested(product, on)
    if refined is not None:
        if multi_models:
            raise ValueError("refined: not with multi_models (a multi-DLA batch cannot be refined)")
        components = tuple(components)
        if "sub_dla" in components:
            raise ValueError("refined: a single-DLA run has no sub-DLA table; components are 'null' and 'dla'")
        by_posteriors = isinstance(model_weights, str)
        if by_posteriors and model_weights != "posteriors":
            raise ValueError("model_weights: 'posteriors', an array [nq, 3] or None")
        if model_weights is not None and not by_posteriors:
            model_weights = np.asarray(model_weights, dtype=np.float64)

        def per_block(batch, idx, lo, hi):
            if by_posteriors:   # (p_no_dlas, 0, p_dlas) of the refine pass this block has just had
                rp = batch.refined_posteriors()
                mw = _posterior_weights(np.stack([rp["p_no_dlas_refined"], np.zeros(rp["p_dlas_refined"].size),
                                                  rp["p_dlas_refined"]], axis=1), components)
            else:
                mw = None if model_weights is None else model_weights[idx]
            return getattr(batch, product)(weights="refined", components=components, model_weights=mw, **kw)
    elif multi_models:
        if not isinstance(p, MultiParameters):
            raise ValueError("multi_models needs MultiParameters (a multi-DLA run)")
        model_weights, multi_rows = _multi_inputs(results, model_weights, multi_rows, posteriors_by_name=True)
        expect = grid_fields.requested("multi_models") + expect

        def per_block(batch, idx, lo, hi):
            return getattr(batch, product + "_multi")(tables=multi_rows(idx), model_weights=model_weights[idx], **on_multi)
    else:
        components, sampled, model_weights, sample_rows = _mixture_inputs(results, components, model_weights, sample_rows)

        def per_block(batch, idx, lo, hi):
            return getattr(batch, product)(weights={c: np.asarray(sample_rows(idx, c), dtype=np.float64) for c in sampled} or None,
                                           components=components, model_weights=None if model_weights is None else model_weights[idx],
                                           **kw)
    return _drive(model, samples, spectra, sel, p, device, max_quasars_per_batch, per_block, expect, refined, plane_dims)


def marginal_continuum(model: dict, samples: dict, spectra, results: dict | None = None,
                       params: Parameters | None = None, selection=None, components=("dla",), model_weights=None,
                       sample_coefficients: bool = False, sample_rows=None, device: int = 0,
                       max_quasars_per_batch: int | None = None, multi_models: bool = False, multi_rows=None,
                       refined: dict | None = None) -> dict:
    """The marginal continuum (:meth:`Batch.marginal_continuum`) of the selected quasars of a processed run,
    batched like :func:`model_spectra`: nothing is swept again, the posterior weights come from the saved
    sample log-likelihoods.

    ``spectra``, ``results``, ``params``, ``selection``: as :func:`model_spectra`.  ``components``: which of
    ``"null"``, ``"sub_dla"`` and ``"dla"`` are mixed.  ``model_weights``: ``[nq, 3]`` over ALL quasars of
    ``spectra`` in the order (null, sub-DLA, DLA), None (equal weights over the listed components) or
    ``"posteriors"``: (p_no_dlas, p_lls or 0, p_dlas) of ``results``, a quasar whose listed posteriors are all
    0 or NaN falling back to equal weights.  The tables are ``sample_log_likelihoods_dla`` (``[nq, S]``, or
    model DLA(1) of ``[nq, max_dlas, S]``) and ``sample_log_likelihoods_lls`` of ``results``;
    ``sample_rows(idx, name) -> [len(idx), S]`` (``name`` ``"dla"`` or ``"sub_dla"``) supplies the rows
    instead (a file streamed block by block).  Returns ``selection``, ``offsets``, ``status`` and the arrays of
    :meth:`Batch.marginal_continuum` in selection order; results do not depend on the batching.  An empty selection returns
    every key the same call returns for a non-empty one, each with no extent (``refined`` and ``multi_models`` included).

    ``multi_models``: the mixture over ALL models of a multi-DLA run instead (:meth:`Batch.marginal_continuum_multi`):
    ``components`` and ``sample_rows`` are ignored, ``results`` must carry ``base_sample_inds``, the 3-D
    ``sample_log_likelihoods_dla`` and ``sample_log_likelihoods_lls`` -- or ``multi_rows(idx)`` returns the dict of those
    three for quasars ``idx`` -- and ``model_weights`` is ``[nq, 2 + max_dlas]`` over ALL quasars (default and
    ``"posteriors"``: ``results["model_posteriors"]``; :func:`renormalised_model_posteriors` includes the quasars of the
    reference's early exit).  The result also carries ``model_flags``; ``sample_coefficients`` are not offered.

    ``refined``: None, or ``dict(levels=, delta=, pad=, points=, prior=)`` (any may be left out): per resident block the
    selected quasars are processed and refined (:meth:`Batch.process`, :meth:`Batch.refine`, the way
    :func:`refine_absorbers` works; ``results`` supplies the priors) and the DLA component runs on the refined table
    (``weights="refined"``: posterior mass outside the last box is ignored); ``model_weights="posteriors"`` then mixes by
    :meth:`Batch.refined_posteriors`.  Components ``"null"`` and ``"dla"`` of single-DLA runs only.  The result gains
    ``boxes`` and ``refine_status``; ``sample_coefficients`` are ``[n, S', k]``."""
    if multi_models and sample_coefficients and refined is None:
        raise ValueError("sample_coefficients are not offered with multi_models")
    return _mixture("marginal_continuum", dict(sample_coefficients=sample_coefficients), model, samples, spectra, results, params,
                    selection, components, model_weights, sample_rows, device, max_quasars_per_batch, multi_models, multi_rows, refined)


def predictive_residuals(pf: dict, flux, kept) -> dict:
    """``residual`` = (y - flux_mean) / sqrt(flux_var + noise_var) per pixel (NaN on masked pixels), and per
    quasar ``chi2`` and ``num_kept``, from what :meth:`Batch.predictive_flux` returns and the observed flux and
    kept flags on the same grid.  The in-sample replicate residual (conservative), not a leave-one-out one."""
    flux, kept = np.asarray(flux, dtype=np.float64), np.asarray(kept, dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        res = np.where(kept, (flux - pf["flux_mean"]) / np.sqrt(pf["flux_var"] + pf["noise_var"]), np.nan)
    off = np.asarray(pf["offsets"])
    n = off.size - 1
    chi2, num = np.full(n, np.nan), np.zeros(n, dtype=np.int64)
    for s in range(n):
        r, kp = res[off[s]:off[s + 1]], kept[off[s]:off[s + 1]]
        num[s] = int(kp.sum())
        chi2[s] = float(np.sum(r[kp] ** 2)) if kp.any() else np.nan
    return {"residual": res, "chi2": chi2, "num_kept": num}


def predictive_flux(model: dict, samples: dict, spectra, results: dict | None = None,
                    params: Parameters | None = None, selection=None, components=("dla",), model_weights=None,
                    residuals: bool = False, sample_rows=None, device: int = 0,
                    max_quasars_per_batch: int | None = None, multi_models: bool = False, multi_rows=None,
                    refined: dict | None = None) -> dict:
    """The posterior predictive flux (:meth:`Batch.predictive_flux`) of the selected quasars of a processed run,
    batched like :func:`marginal_continuum`, whose arguments these are: nothing is swept again, the posterior weights
    come from the saved sample log-likelihoods; ``model_weights="posteriors"`` mixes by
    :func:`posterior_model_weights`.  ``residuals``: also the in-sample replicate ``residual`` per pixel and
    ``chi2``, ``num_kept`` per quasar (conservative; not leave-one-out).  Returns ``selection``, ``offsets``,
    ``status`` and the arrays of :meth:`Batch.predictive_flux` in selection order; results do not depend on the
    batching, and an empty selection returns the same keys with no extent.  ``multi_models``, ``multi_rows``, ``refined``: as :func:`marginal_continuum` (:meth:`Batch.predictive_flux_multi`;
    with ``refined`` the DLA component runs on the refined table, posterior mass outside the last box ignored)."""
    return _mixture("predictive_flux", dict(residuals=residuals), model, samples, spectra, results, params, selection, components,
                    model_weights, sample_rows, device, max_quasars_per_batch, multi_models, multi_rows, refined)


def absorption_distribution(model: dict, samples: dict, spectra, results: dict | None = None,
                            params: Parameters | None = None, selection=None, components=("dla",), model_weights="posteriors",
                            thresholds=(0.8,), bins: int = 64, levels=None, histogram: bool = False, sample_rows=None,
                            device: int = 0, max_quasars_per_batch: int | None = None, multi_models: bool = False,
                            multi_rows=None, refined: dict | None = None) -> dict:
    """The per-pixel distribution of the absorption (:meth:`Batch.absorption_distribution`) of the selected quasars of a
    processed run, block by block like :func:`predictive_flux`, whose shared arguments mean the same here: nothing is
    swept again, the posterior weights come from the saved sample log-likelihoods, ``model_weights="posteriors"`` (the
    default: a mask is a statement about the sightline, not about the DLA model alone) mixes by
    :func:`posterior_model_weights` -- list the components to mix, ``("null", "dla")`` or all three -- and
    ``multi_models`` / ``multi_rows`` / ``refined`` select :meth:`Batch.absorption_distribution_multi` or the refined table.
    ``thresholds``, ``bins``, ``levels``, ``histogram``: as :meth:`Batch.absorption_distribution`.  Returns ``selection``,
    ``offsets``, ``status`` and its arrays in selection order; results do not depend on the batching, and an empty selection
    returns the same keys with no extent.  :func:`forest_mask` cuts the mask."""
    thr = () if thresholds is None else tuple(np.asarray(thresholds, dtype=np.float64).reshape(-1))
    lev = None if levels is None or np.size(levels) == 0 else tuple(np.asarray(levels, dtype=np.float64).reshape(-1))
    kw = dict(thresholds=thr, bins=int(bins), levels=lev, histogram=bool(histogram))
    return _mixture("absorption_distribution", kw, model, samples, spectra, results, params, selection, components, model_weights,
                    sample_rows, device, max_quasars_per_batch, multi_models, multi_rows, refined,
                    plane_dims=dict(thresholds=len(thr), levels=len(lev or ()), bins=int(bins)))


def forest_mask(result: dict, threshold_index: int = 0, probability: float = 0.5) -> np.ndarray:
    """The per-pixel boolean mask ``prob_below[threshold_index] >= probability`` of what
    :func:`absorption_distribution` (or the :class:`Batch` methods) returns: the pixels whose transmission is at or below the
    threshold with at least that posterior probability.  A NaN pixel (a quasar that was not evaluated) is not masked.
    The wings outside the mask are corrected by the caller's division of the flux by ``expected_absorption`` or
    ``mean_absorption`` of :func:`model_spectra`; this function only cuts the mask."""
    p = np.asarray(result["prob_below"], dtype=np.float64)[threshold_index]
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(p), False, p >= probability)


# ----------------------------------------------------------------------------------------------
# mock spectra
# ----------------------------------------------------------------------------------------------

def draw_mock_spectra(model: dict, samples: dict, templates, truth=None, params: Parameters | None = None,
                      seed: int | None = None, first_quasar_index: int = 0, components=(), device: int = 0,
                      max_quasars_per_batch: int | None = None) -> dict:
    """Mock spectra of many quasars, drawn on the GPU from the model the sweeps evaluate
    (:meth:`Batch.draw_mocks`), batched like :func:`process_qsos`.

    ``templates``: list of per-quasar dicts (``wavelengths, flux, noise_variance, pixel_mask, z_qso``):
    the wavelength grids, noise variances and masks of the mocks; a template's flux survives only
    where the model says nothing (outside the modelled rest range, or a quasar the sweep would skip).
    ``truth``: CSR triple ``(offsets [nq + 1], z_dlas, log_nhis)`` over ALL templates
    (:func:`gp_dla_detection_amd.mocks.draw_truth`), or None.  ``params``: a :class:`MultiParameters`
    draws from the mean-flux model.  The Philox key of template i carries ``first_quasar_index + i``
    whatever the batching, so any ``max_quasars_per_batch`` gives the same spectra.
    Returns ``flux`` (list of per-quasar arrays), ``status``, and per requested component a list of
    per-quasar arrays (``latents``: ``[nq, k]``)."""
    p = params or Parameters()
    templates = list(templates)
    nq = len(templates)
    k = np.asarray(model["M"]).shape[1]
    out = {"flux": [], "status": np.zeros(nq, dtype=np.int32)}
    for name in components:
        out[name] = np.empty((nq, k)) if name == "latents" else []
    with closing(_resident_blocks(model, samples, templates, range(nq), p, device, max_quasars_per_batch)) as blocks:
        for lo, hi, idx, batch in blocks:
            batch.ctx.set_first_quasar_index(first_quasar_index + lo)
            res = batch.draw_mocks(absorbers=None if truth is None else _take_absorbers(truth, idx),
                                   seed=seed, write_resident=False, components=components)
            sizes = np.array([np.asarray(t["wavelengths"]).size for t in templates[lo:hi]], dtype=np.int64)
            out["flux"] += split_cells(res["flux"], np.concatenate([[0], np.cumsum(sizes)]))
            out["status"][lo:hi] = res["status"]
            for name in components:
                if name == "latents":
                    out[name][lo:hi] = res[name]
                else:
                    out[name] += split_cells(res[name], res["grid_offsets"])
    return out


def dla_model_mean(model: dict, z_qsos, absorbers=None, suppressed: bool = True, num_voigt_lines: int = 3,
                   num_forest_lines: int = 31, prev_tau_0: float = 0.0023, prev_beta: float = 3.65,
                   device: int = 0) -> np.ndarray:
    """The reference's ``this_mu`` (QSOLoader.plot_this_mu, qso_loader.py:1685-1711) as data on the
    model's rest grid: ``mu`` x (``suppressed``) ``total_scale_factor`` (:1777-1822) x the RAW Voigt
    profiles of each quasar's absorbers at ``rest_wavelengths (1 + z_qso)``.  ``absorbers``: the CSR
    triple ``(offsets [nq + 1], z_dlas, log_nhis)`` of :func:`map_absorbers`, or None.  Returns
    ``[len(z_qsos), G]``."""
    lib = _lib.load()
    z, zp = _f64(np.atleast_1d(z_qsos))
    keep = []
    m = _lib.Model()
    rw, rwp = _f64(model["rest_wavelengths"])
    mu, mup = _f64(model["mu"])
    m.num_rest_pixels, m.k, m.rest_wavelengths, m.mu = rw.size, 0, rwp, mup
    a = SimpleNamespace(absorber_offsets=None, absorber_z=None, absorber_nhi=None)
    _absorber_fields(a, absorbers, z.size, keep, "quasars")
    out = np.empty((z.size, rw.size))
    _lib.check(lib.gpdla_model_mean(C.byref(m), z.size, zp, a.absorber_offsets, a.absorber_z, a.absorber_nhi,
                                    int(num_voigt_lines), int(num_forest_lines),
                                    int(bool(suppressed)), float(prev_tau_0), float(prev_beta),
                                    out.ctypes.data_as(_dp), int(device)))
    return out
