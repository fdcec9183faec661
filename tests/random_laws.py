"""Statistics for the laws of the counter-based random draws (env events, action noise).

Plain module, standard library and numpy only (scipy may be absent where the GPU tests run): the
normal quantile is ``statistics.NormalDist().inv_cdf``, the Kolmogorov-Smirnov threshold comes from
the Kolmogorov series, chi-square quantiles from Wilson-Hilferty, small counts from the exact
binomial law. No threshold is a literal: every one is computed from a false-alarm level and the
sample size.

A test function collects its statistics in one ``Laws`` object and calls ``check()`` once. The total
false-alarm level of the function (``ALPHA`` = 1e-3) is split evenly (Bonferroni) over every
elementary statistic collected: each marginal test, each off-diagonal correlation, each lag, each
equal-fraction comparison counts as one.

The draws are 24-bit uniforms (granularity 6e-8): negligible against 1/sqrt(n) for n <= 2^20, which
is what the Kolmogorov-Smirnov statistic resolves. The extreme-value statistics n (x_min - lo) /
(hi - lo) and n (hi - x_max) / (hi - lo) (each ~ Exp(1)) resolve 1/n, so they are applied only
where the granularity of the recovered draw (``grain``, as a fraction of the range) is far below 1/n.
"""
from __future__ import annotations

import math
from statistics import NormalDist

import numpy as np

ALPHA = 1e-3                  # total false-alarm level of one test function
# No test function collects more statistics than this (``check`` asserts it). The planted-fault tests
# reserve the whole of it, so every plant is caught under thresholds at least as wide as any scenario's.
BUDGET = 1024
LAGS = (1, 2, 4, 16, 64)      # env-index strides: neighbours, team, wave quarter, wave, workgroup
# Upper bound on P(two independent continuous draws are bit-equal). A draw has 2^24 levels; the
# coarsest recovered column is the manager's observation noise on an O(1) value (fp32 spacing 6e-8
# to 1.2e-7 across a width of 0.02: about 2^18 levels). 2^-16 bounds both with room.
P_EQUAL = 2.0 ** -16
U24 = 2.0 ** -24


# ----------------------------------------------------------------------------- quantiles
def normal_quantile(p: float) -> float:
    return NormalDist().inv_cdf(p)


def kolmogorov_sf(lam: float) -> float:
    """P(sqrt(n) D > lam), n -> inf: 2 sum_{k>=1} (-1)^(k-1) exp(-2 k^2 lam^2)."""
    if lam < 0.2:
        return 1.0
    s = 0.0
    for k in range(1, 101):
        t = math.exp(-2.0 * k * k * lam * lam)
        s += t if k % 2 else -t
        if t < 1e-18:
            break
    return min(1.0, max(0.0, 2.0 * s))


def ks_threshold(alpha: float) -> float:
    """lam with kolmogorov_sf(lam) = alpha (bisection)."""
    lo, hi = 0.2, 8.0
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        if kolmogorov_sf(mid) > alpha:
            lo = mid
        else:
            hi = mid
    return hi


def chi2_quantile(df: int, alpha: float) -> float:
    """Upper alpha quantile of chi-square(df): exact for df = 1 (a squared normal), otherwise
    Wilson-Hilferty."""
    if df == 1:
        return normal_quantile(1.0 - 0.5 * alpha) ** 2
    z = normal_quantile(1.0 - alpha)
    c = 2.0 / (9.0 * df)
    return df * (1.0 - c + z * math.sqrt(c)) ** 3


def binomial_two_sided_p(k: int, n: int, p: float) -> float:
    """Two-sided p-value 2 min(P(X <= k), P(X >= k)) of X ~ Binomial(n, p), summed exactly (log
    gamma) over the window around the mean that holds all but ~1e-30 of the mass."""
    mu, sd = n * p, math.sqrt(n * p * (1.0 - p))
    w = int(12.0 * sd + 40.0)
    a, b = max(0, int(mu) - w), min(n, int(mu) + w)
    lp, lq = math.log(p), math.log1p(-p)
    lg = math.lgamma
    pmf = [math.exp(lg(n + 1) - lg(j + 1) - lg(n - j + 1) + j * lp + (n - j) * lq) for j in range(a, b + 1)]
    lower = sum(pmf[:max(0, min(len(pmf), k - a + 1))])
    upper = sum(pmf[max(0, min(len(pmf), k - a)):])
    return min(1.0, 2.0 * min(lower, upper))


def poisson_count_threshold(lam: float, alpha: float) -> int:
    """Smallest c with P(Poisson(lam) > c) <= alpha."""
    term = math.exp(-lam)
    cdf, c = term, 0
    while 1.0 - cdf > alpha and c < 10_000_000:
        c += 1
        term *= lam / c
        cdf += term
    return c


# ----------------------------------------------------------------------------- statistics
def _ks(cdf_sorted: np.ndarray) -> float:
    n = len(cdf_sorted)
    i = np.arange(1, n + 1, dtype=np.float64)
    d = max(float(np.max(i / n - cdf_sorted)), float(np.max(cdf_sorted - (i - 1) / n)))
    return d * math.sqrt(n)


def ks_uniform(x, lo: float, hi: float) -> float:
    """D sqrt(n) of x against U(lo, hi)."""
    u = np.sort((np.asarray(x, np.float64).ravel() - lo) / (hi - lo))
    return _ks(np.clip(u, 0.0, 1.0))


_erf = np.frompyfunc(math.erf, 1, 1)


def normal_cdf(z: np.ndarray) -> np.ndarray:
    return 0.5 * (1.0 + _erf(np.asarray(z, np.float64) / math.sqrt(2.0)).astype(np.float64))


def ks_normal(z) -> float:
    """D sqrt(n) of z against N(0, 1)."""
    return _ks(normal_cdf(np.sort(np.asarray(z, np.float64).ravel())))


def chi2_counts(counts, probs):
    """(Pearson chi-square, degrees of freedom) of observed counts against cell probabilities."""
    c = np.asarray(counts, np.float64)
    e = np.asarray(probs, np.float64) * c.sum()
    return float(((c - e) ** 2 / e).sum()), len(c) - 1


def corr_matrix(cols) -> np.ndarray:
    """|r| sqrt(n) for every pair of columns (zero diagonal). cols: [k][n]."""
    a = np.asarray(cols, np.float64)
    a = a - a.mean(axis=1, keepdims=True)
    a /= np.sqrt((a * a).sum(axis=1, keepdims=True))
    r = np.abs(a @ a.T) * math.sqrt(a.shape[1])
    np.fill_diagonal(r, 0.0)
    return r


def serial_corr(x, lags=LAGS) -> dict:
    """|r| sqrt(n - lag) between x[i] and x[i + lag] over the env index."""
    x = np.asarray(x, np.float64).ravel()
    out = {}
    for lag in lags:
        a, b = x[:-lag] - x[:-lag].mean(), x[lag:] - x[lag:].mean()
        out[lag] = abs(float((a * b).sum() / math.sqrt((a * a).sum() * (b * b).sum()))) * math.sqrt(len(a))
    return out


def equal_fraction(a, b) -> float:
    """Share of bit-equal entries of two arrays that should be independent."""
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    return float(np.count_nonzero(a == b)) / len(a)


# ----------------------------------------------------------------------------- one test's budget
class Laws:
    """The statistics of one test function. Every entry is (name, kind, value, n, extra) with a
    multiplicity (how many elementary statistics it stands for); ``check`` splits ``alpha`` evenly
    over the sum of the multiplicities, computes each threshold from its share and n, prints the
    table and asserts."""

    def __init__(self, alpha: float = ALPHA):
        self.alpha = alpha
        self.rows = []    # (name, kind, value, n, mult, extra)
        self.hard = []    # exact (non-statistical) violations

    def _add(self, name, kind, value, n, mult=1, extra=None):
        self.rows.append((name, kind, float(value), int(n), int(mult), extra))

    # -- marginals
    def uniform(self, name, x, lo, hi, grain: float = U24, slack: float = 0.0):
        """x ~ U(lo, hi): Kolmogorov-Smirnov, the width (second moment about the centre, a z test: with
        t = (2x - lo - hi) / (hi - lo) ~ U(-1, 1), E t^2 = 1/3 and Var t^2 = 4/45; it resolves a range
        scaled about its centre, which moves D by half the scale error only, and needs no 1/n
        granularity), the range itself (exact, up to ``slack``), and, where the draw's granularity
        allows, both extremes."""
        x = np.asarray(x, np.float64).ravel()
        n = len(x)
        if x.min() < lo - slack or x.max() > hi + slack:
            self.hard.append(f"{name}: [{x.min()}, {x.max()}] leaves [{lo}, {hi}]")
        self._add(name, "ks", ks_uniform(x, lo, hi), n)
        t = (2.0 * x - lo - hi) / (hi - lo)
        self._add(name + " width", "z", abs((t * t).mean() - 1.0 / 3.0) * math.sqrt(n / (4.0 / 45.0)), n)
        if grain * n < 0.01:
            self._add(name + " lower end", "extreme", n * (x.min() - lo) / (hi - lo), n)
            self._add(name + " upper end", "extreme", n * (hi - x.max()) / (hi - lo), n)

    def normal(self, name, z):
        """z ~ N(0, 1): Kolmogorov-Smirnov, the mean (z test) and the variance (chi-square)."""
        z = np.asarray(z, np.float64).ravel()
        n = len(z)
        self._add(name, "ks", ks_normal(z), n)
        self._add(name + " mean", "z", abs(z.mean()) * math.sqrt(n), n)
        self._add(name + " variance", "var", ((z - z.mean()) ** 2).sum(), n)

    def discrete(self, name, counts, probs):
        stat, df = chi2_counts(counts, probs)
        self._add(name, "chi2", stat, int(np.sum(counts)), extra=df)

    def bernoulli(self, name, flags, p):
        f = np.asarray(flags).ravel() != 0
        k = int(f.sum())
        self.discrete(name, [k, len(f) - k], [p, 1.0 - p])

    def binomial(self, name, k, n, p):
        """A (small) count against Binomial(n, p), exact two-sided."""
        self._add(name, "binom", binomial_two_sided_p(int(k), int(n), p), n, extra=int(k))

    # -- independence
    def uncorrelated(self, name, cols, names=None):
        """Every pair of the columns ([k][n], or a dict name -> column)."""
        if isinstance(cols, dict):
            names, cols = list(cols), list(cols.values())
        r = corr_matrix(cols)
        k = len(cols)
        i, j = np.unravel_index(int(np.argmax(r)), r.shape)
        tag = f" ({names[i]}, {names[j]})" if names else f" ({i}, {j})"
        self._add(name + tag, "corr", r.max(), len(cols[0]), mult=k * (k - 1) // 2)

    def cross(self, name, a_cols: dict, b_cols: dict):
        """Every column of a against every column of b."""
        a, b = np.asarray(list(a_cols.values()), np.float64), np.asarray(list(b_cols.values()), np.float64)
        a = a - a.mean(axis=1, keepdims=True)
        b = b - b.mean(axis=1, keepdims=True)
        a /= np.sqrt((a * a).sum(axis=1, keepdims=True))
        b /= np.sqrt((b * b).sum(axis=1, keepdims=True))
        r = np.abs(a @ b.T) * math.sqrt(a.shape[1])
        i, j = np.unravel_index(int(np.argmax(r)), r.shape)
        self._add(f"{name} ({list(a_cols)[i]}, {list(b_cols)[j]})", "corr", r.max(), a.shape[1], mult=r.size)

    def serial(self, name, x, lags=LAGS):
        s = serial_corr(x, lags)
        worst = max(s, key=s.get)
        self._add(f"{name} serial (lag {worst})", "corr", s[worst], np.size(x), mult=len(lags))

    def fresh(self, name, a, b, p_equal: float | None = None, shifts=(0, 1, -1)):
        """Two draws of one quantity that should be independent (another call, another seed), aligned
        by env: their correlation, and the share of bit-equal entries, also with the env index shifted
        by one either way (a stream handed to the neighbour). Continuous draws (``p_equal`` None): the
        share against the bound P_EQUAL; discrete ones: the count of equal entries against
        Binomial(n, p_equal), p_equal = sum of the squared cell probabilities, exact and two-sided."""
        a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
        self._add(name + " corr", "corr", corr_matrix([a, b])[0, 1], len(a))
        for s in shifts:
            x, y = (a, b) if s == 0 else (a[:-1], b[1:]) if s > 0 else (a[1:], b[:-1])
            if p_equal is None:
                self._add(f"{name} equal (shift {s})", "equal", equal_fraction(x, y), len(x))
            else:
                self.binomial(f"{name} equal count (shift {s})", int(np.count_nonzero(x == y)), len(x), p_equal)

    def count(self) -> int:
        return sum(r[4] for r in self.rows)

    def reserve(self, total: int = BUDGET):
        """Count further statistics in the split until the budget holds ``total`` of them: a planted-fault
        test takes the thresholds of the largest scenario this way."""
        m = sum(r[4] for r in self.rows)
        if total > m:
            self.rows.append(("(reserved)", "reserved", 0.0, 0, total - m, None))

    def exact(self, name, ok: bool):
        if not ok:
            self.hard.append(name)

    # -- verdict
    def evaluate(self):
        """[(name, kind, value, threshold, ok)] with the level split over all elementary statistics."""
        m = sum(r[4] for r in self.rows)
        a = self.alpha / max(m, 1)
        out = []
        for name, kind, v, n, _, extra in self.rows:
            if kind == "ks":
                thr = ks_threshold(a)
                ok = v <= thr
            elif kind in ("corr", "z"):
                thr = normal_quantile(1.0 - 0.5 * a)
                ok = v <= thr
            elif kind == "extreme":   # Exp(1): too far from the end (the end is never passed: exact check)
                thr = -math.log(a)
                ok = v <= thr
            elif kind == "chi2":
                thr = chi2_quantile(extra, a)
                ok = v <= thr
            elif kind == "var":       # sum of squares ~ chi-square(n - 1), two-sided
                lo, hi = chi2_quantile(n - 1, 1.0 - 0.5 * a), chi2_quantile(n - 1, 0.5 * a)
                thr = hi / (n - 1)
                ok = lo <= v <= hi
                v = v / (n - 1)
            elif kind == "binom":     # value is the p-value
                thr = a
                ok = v >= thr
            elif kind == "equal":
                thr = poisson_count_threshold(n * P_EQUAL, a) / n
                ok = v <= thr
            elif kind == "reserved":
                continue
            else:
                raise ValueError(kind)
            out.append((name, kind, v, thr, ok))
        return out

    def failures(self):
        return [r[0] for r in self.evaluate() if not r[4]] + list(self.hard)

    def report(self, title: str = "") -> str:
        rows = self.evaluate()
        lines = [f"-- {title}: {len(rows)} entries, {sum(r[4] for r in self.rows)} statistics, alpha {self.alpha:g}"]
        for name, kind, v, thr, ok in rows:
            lines.append(f"   {'ok  ' if ok else 'FAIL'} {kind:8s} {v:12.5g}  (threshold {thr:10.5g})  {name}")
        lines += [f"   FAIL exact {h}" for h in self.hard]
        return "\n".join(lines)

    def summary(self) -> dict:
        """Largest value per kind, with its threshold (for the design notes)."""
        out = {}
        for name, kind, v, thr, ok in self.evaluate():
            if kind not in out or (v > out[kind][0] if kind != "binom" else v < out[kind][0]):
                out[kind] = (v, thr)
        return out

    def check(self, title: str = ""):
        print(self.report(title))
        assert self.count() <= BUDGET, (self.count(), BUDGET)
        bad = self.failures()
        assert not bad, bad
