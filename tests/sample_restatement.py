"""NumPy / SciPy restatement of generate_dla_samples.m, multi_dlas/generate_dla_samples_multi.m and
multi_dlas/set_lls_parameters.m as written: ksdensity's default normal-kernel estimate, polyfit of
its logarithm in raw t, adaptive quadrature for Z and the CDF, a bracketing root finder for the
inverse.  The quasi-random stream is the reverse-radix ("RR2") scrambled Halton set in exact
rational arithmetic.  The CPU reference of tests/test_samples.py and tests/test_gpu_samples.py."""
from fractions import Fraction

import numpy as np
from scipy.integrate import quad
from scipy.optimize import brentq

UPPER = 25.0
LLS_BREAK = 20.03269   # set_lls_parameters.m:48-49


def make_catalogue():
    rng = np.random.default_rng(1)
    v = 20 + rng.exponential(0.45, 6000)
    return v[v < 22.8]


def rr2_permutation(b):
    m = (b - 1).bit_length()
    out = []
    for v in range(1 << m):
        r = sum(((v >> bit) & 1) << (m - 1 - bit) for bit in range(m))
        if r < b:
            out.append(r)
    return out


def radical_inverse(index, b):
    """Sum_j pi_b(d_j) b^-(j+1) over the base-b digits of index, exactly."""
    perm, x, scale = rr2_permutation(b), Fraction(0), Fraction(1, b)
    while index > 0:
        index, d = divmod(index, b)
        x += perm[d] * scale
        scale /= b
    return x


def halton(first_index, num, bases=(2, 3, 5)):
    return np.array([[float(radical_inverse(i, b)) for b in bases] for i in range(first_index, first_index + num)],
                    dtype=np.float64).reshape(num, len(bases))


def bandwidth(v):
    v = np.asarray(v, dtype=np.float64)
    sig = np.median(np.abs(v - np.median(v))) / 0.6745
    return sig * (4.0 / (3.0 * v.size)) ** (1.0 / 5.0)


def ksdensity(v, x, h=None):
    v, x = np.asarray(v, dtype=np.float64), np.asarray(x, dtype=np.float64)
    h = bandwidth(v) if h is None else h
    out = np.empty(x.size)
    for i0 in range(0, x.size, 128):   # (bounded memory)
        z = (x[i0:i0 + 128, None] - v[None, :]) / h
        out[i0:i0 + 128] = np.exp(-0.5 * z * z).sum(axis=1) / (v.size * h * np.sqrt(2 * np.pi))
    return out


def fit_grid(fit_min=20.0, fit_max=22.0):
    return np.linspace(fit_min, fit_max, 1000)


def fit_raw(x, kde_pdf):
    """f = polyfit(x, log(kde_pdf), 2): highest power first, raw t."""
    return np.polyfit(x, np.log(kde_pdf), 2)


def fit_centred(x, kde_pdf):
    """The same least-squares problem about the middle of the grid; returns (coefficients, centre)."""
    c = 0.5 * (x[0] + x[-1])
    return np.polyfit(x - c, np.log(kde_pdf), 2), c


class Prior:
    """normalized_pdf and cdf of the scripts.  ``lls``: set_lls_parameters.m (flat below the break,
    lower limit 19.5, uniform on 19.5 .. 23, alpha 0.97)."""

    def __init__(self, log_nhis, alpha=0.9, uniform=(20.0, 23.0), fit=(20.0, 22.0), lls=False):
        self.x = fit_grid(*fit)
        self.kde = ksdensity(log_nhis, self.x)
        self.f = fit_raw(self.x, self.kde)
        self.lls = lls
        if lls:
            alpha, uniform = 0.97, (19.5, 23.0)
        self.alpha, self.umin, self.umax = alpha, uniform[0], uniform[1]
        self.lower = 19.5 if lls else fit[0]
        self.breaks = sorted({self.umin, self.umax} | ({LLS_BREAK} if lls else set()))
        self.Z = self._quad(self.g, self.lower, UPPER)
        self._knots = [self.lower] + [b for b in self.breaks if self.lower < b < UPPER]
        self._F_knots = np.concatenate([[0.0], np.cumsum([self._quad(self.pdf, a, b) for a, b in
                                                          zip(self._knots[:-1], self._knots[1:])])])

    def _quad(self, fn, a, b):
        pts = [p for p in self.breaks if a < p < b]
        return quad(fn, a, b, points=pts or None, epsabs=1e-13, epsrel=1e-13, limit=200)[0]

    def g(self, t):
        if self.lls and t < LLS_BREAK:
            t = LLS_BREAK
        return np.exp(np.polyval(self.f, t))

    def pdf(self, t):
        u = 1.0 / (self.umax - self.umin) if self.umin <= t <= self.umax else 0.0
        return self.alpha * (self.g(t) / self.Z) + (1 - self.alpha) * u

    def cdf(self, x):
        """integral(normalized_pdf, lower, x): the smooth pieces up to the last break point below x,
        then one quadrature of the rest."""
        if x <= self.lower:
            return 0.0
        k = max(i for i, a in enumerate(self._knots) if a < x)
        return self._F_knots[k] + quad(self.pdf, self._knots[k], x, epsabs=1e-13, epsrel=1e-13, limit=200)[0]

    def inverse(self, u, bracket=None):
        """The root of cdf(x) = u on [lower, 25] (fzero of the scripts, here bracketed).  ``bracket``: a
        narrower interval to try first; it is used only if the root lies inside."""
        if u <= 0.0:
            return self.lower
        if u >= self.cdf(UPPER):
            return UPPER
        h = lambda x: self.cdf(x) - u
        if bracket is not None:
            a, b = max(bracket[0], self.lower), min(bracket[1], UPPER)
            if a < b and h(a) < 0.0 < h(b):
                return brentq(h, a, b, xtol=1e-15, rtol=8.9e-16)
        return brentq(h, self.lower, UPPER, xtol=1e-15, rtol=8.9e-16)


def generate(log_nhis, num, alpha=0.9, lls=False):
    """The variables the scripts save, from the restated stream."""
    seq = halton(0, num)
    prior = Prior(log_nhis, alpha)
    log_nhi = np.array([prior.inverse(u) for u in seq[:, 1]])
    out = dict(offset_samples=seq[:, 0], log_nhi_samples=log_nhi, nhi_samples=10.0 ** log_nhi)
    if lls:
        lp = Prior(log_nhis, lls=True)
        l = 19.5 + (20.0 - 19.5) * seq[:, 2]
        out.update(lls_log_nhi_samples=l, lls_nhi_samples=10.0 ** l,
                   Z_lls=lp.cdf(20.0) - lp.cdf(19.5), Z_dla=lp.cdf(23.0) - lp.cdf(20.0))
    return out
