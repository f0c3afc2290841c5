"""DLA parameter samples and LLS normalisers from a catalogue's log10 N_HI values, on the GPU.

Restates ``generate_dla_samples.m``, ``multi_dlas/generate_dla_samples_multi.m`` and
``multi_dlas/set_lls_parameters.m``: quasi-random points of a Halton set
scrambled by the reverse-radix rule, a kernel density estimate of the catalogue's log N_HI, a
quadratic through its logarithm, the mixture of that fit with a uniform density, and inverse
transform sampling of the mixture.  Every number is computed by libgpdla (csrc/sample_kernels.hpp);
there is no CPU path.

Command line::

    python -m gp_dla_detection_amd.samples LOG_NHIS OUT [--multi] [--lls] [--num N] [--device D]

``LOG_NHIS`` is an ``.npz`` or ``.mat`` file holding a plain vector ``log_nhis``, or a text file of
numbers.  The reference keeps these values inside a ``containers.Map`` in ``catalog.mat``
(generate_dla_samples.m:26-28), which HDF5 stores opaquely and ``io.load_catalog`` declines: export
them from MATLAB as ``log_nhis = cat(1, all_log_nhis{ind}); save('log_nhis.mat', 'log_nhis',
'-v7.3')``, the way the ``--prior`` file of ``run_dr12q`` is exported.  ``OUT`` is the
``dla_samples.mat`` the drivers read; with ``--lls`` it also carries ``Z_lls`` and ``Z_dla``, which
``run_dr12q --multi`` then takes from it.
"""
from __future__ import annotations

import argparse
import ctypes as C
import math
from dataclasses import dataclass, replace

import numpy as np

from . import _lib

UPPER_LOG_NHI = 25.0   # upper limit of every integral of the three scripts (generate_dla_samples.m:38)


@dataclass(frozen=True)
class SampleParameters:
    """The constants of the column density prior.  Defaults: the single-DLA run."""
    num_dla_samples: int = 10000          # set_parameters.m:48
    alpha: float = 0.9                    # :49  weight of the fitted component
    uniform_min_log_nhi: float = 20.0     # :50
    uniform_max_log_nhi: float = 23.0     # :51
    fit_min_log_nhi: float = 20.0         # :52
    fit_max_log_nhi: float = 22.0         # :53
    # the sub-DLA model (multi_dlas/set_lls_parameters.m)
    min_lls_log_nhi: float = 19.5         # set_lls_parameters.m:6
    lls_alpha: float = 0.97               # :5
    lls_uniform_min_log_nhi: float = 19.5     # :7
    lls_uniform_max_log_nhi: float = 23.0     # :8
    extrapolate_min_log_nhi: float = 19.5     # :11
    lls_break_log_nhi: float = 20.03269       # :48-49  below it the fitted density is held constant

    @classmethod
    def single(cls) -> "SampleParameters":
        """set_parameters.m:48-53"""
        return cls()

    @classmethod
    def multi(cls) -> "SampleParameters":
        """multi_dlas/set_parameters_multi.m:48-53"""
        return cls(alpha=0.97)

    def lls(self) -> "SampleParameters":
        """The mixture set_lls_parameters.m:5-11 normalises: its alpha, uniform range and lower limit."""
        return replace(self, alpha=self.lls_alpha, uniform_min_log_nhi=self.lls_uniform_min_log_nhi,
                       uniform_max_log_nhi=self.lls_uniform_max_log_nhi)


def rr2_permutation(b: int) -> tuple:
    """The reverse-radix permutation of the digits 0 .. b-1: the ceil(log2 b)-bit bit reversals of
    0, 1, 2, ... in order, those >= b dropped.  (0, 1); (0, 2, 1); (0, 4, 2, 1, 3); ..."""
    b = int(b)
    if b < 2:
        raise ValueError("base must be >= 2")
    m = (b - 1).bit_length()
    rev = (int(format(v, f"0{m}b")[::-1], 2) for v in range(1 << m))
    return tuple(r for r in rev if r < b)


def _vec(a, name):
    v = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))
    if not np.all(np.isfinite(v)):
        raise ValueError(f"{name} holds values that are not finite")
    return v


def scrambled_halton(first_index: int, num: int, bases=(2, 3, 5), device: int = 0) -> np.ndarray:
    """Points ``first_index .. first_index + num - 1`` of the RR2-scrambled Halton set with the given
    bases, ``[num, len(bases)]``.  Index 0 is the origin (the reference's ``sequence(1, :)``).  Each
    coordinate is the correctly rounded value of an exact rational, so the points are bit-reproducible."""
    lib = _lib.load()
    b = np.ascontiguousarray(np.asarray(bases, dtype=np.int32).reshape(-1))
    out = np.empty((max(int(num), 0), b.size), dtype=np.float64)
    _lib.check(lib.gpdla_samples_halton(int(first_index), int(num), int(b.size), b.ctypes.data_as(_lib._i32p),
                                        _lib.ptr(out), int(device)))
    return out


def kde(values, points, bandwidth: float | None = None, device: int = 0, return_bandwidth: bool = False):
    """``ksdensity(values, points)`` with its defaults: a normal kernel, no boundary correction,
    bandwidth ``sig (4 / (3 N))^(1/5)`` with ``sig = median(|v - median(v)|) / 0.6745`` unless one is
    passed.  ``return_bandwidth``: also return the bandwidth used."""
    lib = _lib.load()
    v, x = _vec(values, "values"), _vec(points, "points")
    out = np.empty_like(x)
    h = C.c_double(0.0)
    _lib.check(lib.gpdla_samples_kde(v.size, _lib.ptr(v), x.size, _lib.ptr(x), 0.0 if bandwidth is None else float(bandwidth),
                                     _lib.ptr(out), C.byref(h), int(device)))
    out = out.reshape(np.shape(points))
    return (out, h.value) if return_bandwidth else out


class NhiPrior:
    """p(t) = alpha g(t) / Z + (1 - alpha) U[uniform_min, uniform_max](t) on [lower, 25], with
    log g a quadratic about ``centre`` (``coeff``: constant, linear, quadratic) and, with a
    ``flat_below``, g held at g(flat_below) below it."""

    def __init__(self, struct: _lib.NhiPrior, device: int = 0):
        self._s = struct
        self.device = int(device)

    coeff = property(lambda self: tuple(self._s.coeff))
    centre = property(lambda self: self._s.centre)
    alpha = property(lambda self: self._s.alpha)
    uniform_min = property(lambda self: self._s.uniform_min)
    uniform_max = property(lambda self: self._s.uniform_max)
    lower = property(lambda self: self._s.lower)
    flat_below = property(lambda self: self._s.flat_below)
    Z = property(lambda self: self._s.Z)

    def polyfit_coefficients(self) -> np.ndarray:
        """The quadratic in raw t, highest power first, as MATLAB's ``polyfit`` returns it (for display:
        evaluate with ``coeff`` about ``centre``)."""
        c0, c1, c2 = self.coeff
        m = self.centre
        return np.array([c2, c1 - 2 * c2 * m, c0 - c1 * m + c2 * m * m])

    def _eval(self, x, want_pdf):
        lib = _lib.load()
        v = _vec(x, "x")
        out = np.empty_like(v)
        args = (_lib.ptr(out), None) if want_pdf else (None, _lib.ptr(out))
        _lib.check(lib.gpdla_samples_prior_eval(C.byref(self._s), v.size, _lib.ptr(v), *args, self.device))
        return out.reshape(np.shape(x)) if np.ndim(x) else float(out[0])

    def pdf(self, x):
        return self._eval(x, True)

    def cdf(self, x):
        """F(x), the integral of the density from ``lower`` to x."""
        return self._eval(x, False)


def fit_nhi_prior(log_nhis, params: SampleParameters | None = None, lls: bool = False, bandwidth: float | None = None,
                  device: int = 0) -> NhiPrior:
    """The prior of generate_dla_samples.m:30-46 fitted to ``log_nhis``; ``lls=True``: the one of
    set_lls_parameters.m:39-56 (``params.lls()``'s mixture on [19.5, 25], flat below 20.03269)."""
    lib = _lib.load()
    p = params or SampleParameters()
    v = _vec(log_nhis, "log_nhis")
    s = _lib.NhiPrior()
    if lls:
        q = p.lls()
        lower, flat = p.extrapolate_min_log_nhi, p.lls_break_log_nhi
    else:
        q, lower, flat = p, p.fit_min_log_nhi, math.nan
    _lib.check(lib.gpdla_samples_fit_prior(v.size, _lib.ptr(v), q.fit_min_log_nhi, q.fit_max_log_nhi, q.alpha,
                                           q.uniform_min_log_nhi, q.uniform_max_log_nhi, lower, flat,
                                           0.0 if bandwidth is None else float(bandwidth), C.byref(s), int(device)))
    return NhiPrior(s, device)


def generate_dla_samples(log_nhis, params: SampleParameters | None = None, multi: bool = False, lls: bool = False,
                         sequence=None, num: int | None = None, first_index: int = 0, device: int = 0) -> dict:
    """``dla_samples.mat`` from the catalogue's log N_HI values.

    Returns what :func:`io.load_dla_samples` returns (``offset_samples``, ``log_nhi_samples``,
    ``nhi_samples``) plus the scalars the reference saves (``alpha``, ``uniform_min_log_nhi``,
    ``uniform_max_log_nhi``, ``fit_min_log_nhi``, ``fit_max_log_nhi``; generate_dla_samples.m:59-61).
    ``multi``: the constants of set_parameters_multi.m when ``params`` is not given.  ``lls=True`` adds
    what set_lls_parameters.m computes -- ``lls_log_nhi_samples``, ``lls_nhi_samples``, ``Z_lls``,
    ``Z_dla`` -- from the third coordinate and the LLS mixture; the DLA samples stay those of ``params``.
    ``sequence``: an ``[S, 2]`` (``lls``: ``[S, 3]``) array of uniforms used instead of the built-in
    scrambled Halton points ``first_index .. first_index + num - 1``."""
    lib = _lib.load()
    p = params or (SampleParameters.multi() if multi else SampleParameters.single())
    prior = fit_nhi_prior(log_nhis, p, device=device)
    seq_ptr, dims = None, 0
    if sequence is not None:
        seq = np.ascontiguousarray(np.asarray(sequence, dtype=np.float64))
        if seq.ndim != 2 or seq.shape[1] not in (2, 3):
            raise ValueError("sequence must be [S, 2] or [S, 3]")
        if num is not None and int(num) != seq.shape[0]:
            raise ValueError("num and the sequence disagree")
        S, dims, seq_ptr = seq.shape[0], seq.shape[1], _lib.ptr(seq)
    else:
        S = int(p.num_dla_samples if num is None else num)
    names = ("offset_samples", "log_nhi_samples", "nhi_samples") + (
        ("lls_offset_samples", "lls_log_nhi_samples", "lls_nhi_samples") if lls else ())
    arrays = {n: np.empty(max(S, 0), dtype=np.float64) for n in names}
    draw = _lib.SampleDraw(*[_lib.ptr(arrays[n]) for n in names])
    _lib.check(lib.gpdla_samples_draw(C.byref(prior._s), int(first_index), S, seq_ptr, dims, p.min_lls_log_nhi,
                                      p.fit_min_log_nhi, C.byref(draw), int(device)))
    out = {n: arrays[n] for n in names if n != "lls_offset_samples"}
    out.update(alpha=p.alpha, uniform_min_log_nhi=p.uniform_min_log_nhi, uniform_max_log_nhi=p.uniform_max_log_nhi,
               fit_min_log_nhi=p.fit_min_log_nhi, fit_max_log_nhi=p.fit_max_log_nhi)
    if lls:
        lp = fit_nhi_prior(log_nhis, p, lls=True, device=device)
        F = lp.cdf(np.array([p.min_lls_log_nhi, p.fit_min_log_nhi, lp.uniform_max]))
        out.update(Z_lls=float(F[1] - F[0]), Z_dla=float(F[2] - F[1]))   # set_lls_parameters.m:70-71
    return out


def load_log_nhis(path: str) -> np.ndarray:
    """A plain ``log_nhis`` vector from an ``.npz`` or ``.mat`` file, or a text file of numbers."""
    from . import io
    if path.endswith(".npz"):
        with np.load(path) as f:
            return np.asarray(f["log_nhis"], dtype=np.float64).reshape(-1)
    if path.endswith(".mat"):
        m = io._load_mat(path, ("log_nhis",))
        if "log_nhis" not in m or not isinstance(m["log_nhis"], np.ndarray) or m["log_nhis"].dtype.kind not in "fiu":
            raise KeyError(f"{path} holds no plain numeric vector log_nhis (a containers.Map cannot be read: see "
                           "the module documentation)")
        return np.asarray(m["log_nhis"], dtype=np.float64).reshape(-1)
    return np.loadtxt(path, dtype=np.float64).reshape(-1)


def main(argv=None):
    from . import io
    ap = argparse.ArgumentParser(description="dla_samples.mat from a catalogue's log10 N_HI values (see the module documentation)")
    ap.add_argument("log_nhis", help=".npz / .mat with a vector log_nhis, or a text file")
    ap.add_argument("out", help="dla_samples.mat to write (-v7.3)")
    ap.add_argument("--multi", action="store_true", help="constants of set_parameters_multi.m (alpha 0.97)")
    ap.add_argument("--lls", action="store_true", help="also the LLS samples and Z_lls / Z_dla (set_lls_parameters.m)")
    ap.add_argument("--num", type=int, default=None, help="number of samples (default 10000)")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    samples = generate_dla_samples(load_log_nhis(args.log_nhis), multi=args.multi, lls=args.lls, num=args.num,
                                   device=args.device)
    io.save_dla_samples(args.out, samples)
    extra = f", Z_lls = {samples['Z_lls']:.6f}, Z_dla = {samples['Z_dla']:.6f}" if args.lls else ""
    print(f"{args.out}: {samples['offset_samples'].size} samples{extra}")


if __name__ == "__main__":
    main()
