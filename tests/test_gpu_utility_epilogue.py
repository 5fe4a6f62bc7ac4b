# -*- coding: utf-8 -*-
"""MI355X: the last step of the sweep -- (mu, sigma^2) -> utility -> arg-min -- at every place util_value() is emitted
from, judged against the device's OWN mu and sigma^2 (``return_all=True``), so the tolerance is the forward-error bound of
the utility formula in fp64 (tests/util_ref.py: a few ulps of its terms) and not the GP's cond(K)-sized one.

Per emission site (the shapes follow launch_sweep: 256 persistent workgroups of 64 candidates, 256-row blocks, a last
round of at most 184 blocks split by row block), per utility, with and without the box / mask gate:

  * every admissible candidate is compared in VALUE (|u - truth(mu, var)| <= bound(mu, var)) or in CLASS (NaN / +inf /
    0.0 as the reference's fp64 code gives them); every inadmissible one must be exactly +inf; nothing is left out;
  * the arrays have exactly m entries;
  * a row with a NaN coordinate is inadmissible with or without a gate (mu = var = NaN, u = +inf);
  * (best_index, best_u) is the arg-min of the returned u (ties to the lowest index, NaN and +inf never win), bit for
    bit.

The models are nearly uncorrelated training sets (length scale below the point spacing) so that a candidate at r length
scales from a training point has sigma^2 ~ amp (1 - exp(-r^2)) + exp(white_noise): r drawn log-uniformly walks sigma^2
from the rounding level of ``amp - q`` (where the device's sigma^2 comes out <= 0 now and then) up to amp; Jones's z is
steered by dedicated rows and by zeta.  The occupancy of every sigma^2 decade, z bin and class is ASSERTED per site and
utility, so that a change of the inputs cannot hollow the test out; the seeds were chosen on the CPU with
oracle/george_oracle.py so that the oracle's (mu, sigma^2) alone gives twice the required counts.

Worst err / bound per site and utility is printed (pytest -s) and recorded in DESIGN.md."""
import collections

import numpy as np
import pytest

import fantasy_ref
import util_ref as ur

pytestmark = pytest.mark.gpu

MIN_COUNT = 20
Case = collections.namedtuple("Case", "n D m form amp wn offset lin seed q")


def C(n, D, m, form, amp, wn, offset, lin=None, seed=0, q=0):
    return Case(n, D, m, form, amp, wn, offset, lin, seed, q)


# site -> cases.  D runs over 1, 2, 3, 5, 8, 16, 17, 32 (every DPAD instantiation emits).
SITES = {
    # persistent kernel, inverse form, one row block (n <= 256)
    "persistent-inverse-1rb": [C(50, 1, 3000, "inverse", 1.0, -30, 1.0, seed=1),
                               C(200, 2, 3000, "inverse", 1e3, -30, 1e3, seed=2),
                               C(50, 1, 3000, "inverse", 1e-6, -30, 1e-3, seed=3),
                               C(200, 2, 3000, "inverse", 1.0, -20, -1.0, seed=4),
                               C(50, 1, 1, "inverse", 1.0, -12, 1.0, seed=5), C(50, 1, 63, "inverse", 1.0, -12, 1.0, seed=6),
                               C(50, 1, 65, "inverse", 1.0, -20, 1.0, seed=7), C(200, 2, 1, "inverse", 1e3, -30, 1.0, seed=8),
                               C(200, 2, 63, "inverse", 1e3, -30, 1e3, seed=9), C(200, 2, 65, "inverse", 1.0, -30, 1.0, seed=10)],
    # several row blocks, 469 candidate blocks: remainder 213 > 184, no split launch
    "persistent-inverse-multi": [C(1152, 8, 30000, "inverse", 1e3, -30, 1.0, seed=11)],
    # 79 candidate blocks, all in the split launch + sweep_finish_kernel
    "split-only": [C(1100, 3, 5000, "inverse", 1e3, -30, -1e3, seed=12)],
    # 625 candidate blocks: 512 persistent + 113 split
    "persistent-plus-split": [C(1100, 5, 40000, "inverse", 1e3, -30, 1e-3, seed=13)],
    "solve-static-diagonal": [C(1152, 16, 3000, "solve", 1e3, -30, 1.0, seed=14)],
    "solve-dynamic": [C(2100, 17, 3000, "solve", 1e3, -30, -1.0, seed=15)],
    # sweep2_kernel<*, true, *>: 256 persistent + 79 split blocks (the finish kernel's fma(lin_coef, ktl, amp)), and solve
    "linear-term": [C(1100, 32, 21384, "inverse", 1e3, -30, 1.0, lin=1, seed=16),
                    C(300, 3, 3000, "solve", 1e3, -30, 1.0, lin=2, seed=17)],
    "fantasy": [C(200, 2, 3000, "inverse", 1e3, -30, 1.0, seed=18, q=3),
                C(300, 8, 3000, "solve", 1e3, -30, 1e3, seed=19, q=3)],
}
BASE_ROWS = 5000        # distinct candidate rows of a large case (tiled up to m: repeated rows are judged once)


def make_gp(mod, case, ell):
    D = case.D
    k = mod.ExpSquaredKernel(np.full(D, ell * ell), ndim=D)
    if case.amp != 1.0:
        k = float(case.amp) * k
    if case.lin:
        k = k + 0.3 * mod.kernels.LinearKernel(log_gamma2=0.4, order=case.lin, bounds=None, ndim=D)
    return mod.GP(kernel=k, fit_mean=True, mean=float(case.offset), white_noise=float(case.wn), fit_white_noise=False)


def build_case(case):
    """Training set, observations, candidate matrix, mask, box and the Jones zetas of one case (host only)."""
    rs = np.random.RandomState(1000 + case.seed)
    n, D, m = case.n, case.D, case.m
    X = rs.uniform(-1.0, 1.0, size=(n, D))
    nn = np.empty(n)
    for i0 in range(0, n, 256):
        d2 = ((X[i0:i0 + 256, None, :] - X[None, :, :]) ** 2).sum(-1)
        d2[np.arange(len(d2)), i0 + np.arange(len(d2))] = np.inf
        nn[i0:i0 + 256] = np.sqrt(d2.min(axis=1))
    ell = 0.5 * np.percentile(nn, 5)
    sa = np.sqrt(case.amp)
    spread = 0.2 * sa
    h = rs.uniform(-1.0, 1.0, size=n)
    y = case.offset + spread * h
    ybest = float(np.max(y))
    zeta_neg = 0.05 * sa                        # imp < 0 everywhere: z < 0
    zeta_pos = -(2.0 * spread + 0.05 * sa)      # imp > 0 everywhere: z > 0
    nb = min(m, BASE_ROWS)

    def near(i, r):
        d = rs.normal(size=(len(i), D))
        d /= np.sqrt((d * d).sum(axis=1))[:, None]
        return X[i] + (r * ell)[:, None] * d

    rows = []
    if nb >= 1000:
        # sigma^2 ladder: log-uniform from the rounding level to amp
        k = int(0.45 * nb)
        v = 10.0 ** rs.uniform(-13.5, np.log10(case.amp) - 0.01, size=k)
        r = np.sqrt(-np.log1p(-np.minimum(v / case.amp, 0.99)))
        rows.append(near(rs.randint(n, size=k), r))
        # training points themselves
        rows.append(X[rs.randint(n, size=int(0.08 * nb))])
        # z rows: (point, r) pairs whose z -- by the uncorrelated approximation -- fills every unit bin of [-9, 9]
        for zeta in (zeta_neg, zeta_pos):
            i = rs.randint(n, size=40000)
            r = 10.0 ** rs.uniform(-3.0, 0.3, size=40000)
            z = (case.offset + (y[i] - case.offset) * np.exp(-0.5 * r * r) - ybest - zeta) / (sa * np.sqrt(-np.expm1(-r * r)))
            keep = []
            per = max(8, int(0.011 * nb))
            for b in range(-9, 9):
                keep.append(np.nonzero((z >= b) & (z < b + 1))[0][:per])
            keep = np.concatenate(keep)
            rows.append(near(i[keep], r[keep]))
        have = sum(len(a) for a in rows)
        rows.append(rs.uniform(-1.25, 1.25, size=(nb - have, D)))      # anywhere, some outside the box
        T = np.concatenate(rows)[rs.permutation(nb)]
    else:
        i = rs.randint(n, size=nb)
        T = near(i, 10.0 ** rs.uniform(-7.0, 0.0, size=nb))
        T[::7] = X[i[::7]]
    T = np.ascontiguousarray(np.tile(T, ((m + nb - 1) // nb, 1))[:m])
    if m > 8:
        T[0, 0] = np.nan                        # the lowest index of all: see test_nan_row_never_wins
        T[m - 2, D - 1] = np.nan
        T[5, D - 1] = 1.5                       # outside the box
        T[m - 1, 0] = -1.5
    mask = (rs.uniform(size=m) > 0.05).astype(np.uint8)
    box = [(-1.1, 1.1)] * D
    return dict(X=X, y=y, T=T, mask=mask, box=box, ell=ell, ybest=ybest, zetas=(zeta_neg, zeta_pos))


class Occupancy(object):
    """Counts of what was compared, per utility: sigma^2 decades and Jones z bins of the value-compared rows, classes."""

    def __init__(self):
        self.decade = collections.defaultdict(collections.Counter)
        self.zbin = collections.Counter()
        self.classes = collections.defaultdict(collections.Counter)
        self.worst = collections.defaultdict(float)
        self.amp = 0.0

    def add(self, kind, classes, ratios, var, z):
        classes = np.asarray(classes)
        val = classes == "value"
        with np.errstate(all="ignore"):
            dec = np.floor(np.log10(var[val]))
        for d, c in zip(*np.unique(dec[np.isfinite(dec)], return_counts=True)):
            self.decade[kind][int(d)] += int(c)
        if kind == "jones":
            zb = np.clip(np.floor(z[val]), -9, 8)
            for b, c in zip(*np.unique(zb[np.isfinite(zb)], return_counts=True)):
                self.zbin[int(b)] += int(c)
        for c, k in zip(*np.unique(classes, return_counts=True)):
            self.classes[kind][str(c)] += int(k)
        if val.any():
            self.worst[kind] = max(self.worst[kind], float(np.max(ratios[val])))

    def check(self, site):
        top = int(np.ceil(np.log10(min(self.amp, 1e2)))) - 1
        for kind in ur.KINDS:
            print("[%s] %-5s worst err/bound %.3f  classes %s" % (site, kind, self.worst[kind], dict(self.classes[kind])))
            low = [d for d in range(-12, top + 1) if self.decade[kind][d] < MIN_COUNT]
            assert not low, (site, kind, "sigma^2 decades short of %d rows" % MIN_COUNT, low, dict(self.decade[kind]))
        lowz = [b for b in range(-9, 9) if self.zbin[b] < MIN_COUNT]        # -9: z < -8, 8: z >= 8
        assert not lowz, (site, "Jones z bins short of %d rows" % MIN_COUNT, lowz, dict(self.zbin))
        seen = collections.Counter()
        for kind in ur.KINDS:
            seen.update(self.classes[kind])
        for cls in ("nan", "+inf", "zero", "inadmissible"):
            assert seen[cls] > 0, (site, "no row of class", cls, dict(seen))


def nan_rows(T):
    return np.isnan(T).any(axis=1)


def contract_argmin(u, T):
    """The arg-min contract of include/apgp.h on a returned u (a row with a NaN coordinate never wins: its u is +inf)."""
    return fantasy_ref.argmin(np.where(nan_rows(T), np.inf, u))


def check_call(site, kind, zeta, ybest, T, box, mask, res, occ, fantasy=False):
    bi, bu, u, mu, var = res
    m = len(T)
    assert u.shape == mu.shape == var.shape == (m,)
    bad = nan_rows(T)
    adm = fantasy_ref.admissible(T, box, mask) & ~bad      # (include/apgp.h: a NaN row is inadmissible, gate or not)
    assert np.all(np.isposinf(u[~adm])), (site, kind, "inadmissible rows must be +inf")
    assert np.all(np.isnan(mu[bad])) and np.all(np.isnan(var[bad]))
    # (a fantasy pick whose sigma^2 + white noise came out <= 0 leaves NaN variances behind: judged by class below)
    assert not np.any(np.isnan(mu[~bad])) and (fantasy or not np.any(np.isnan(var[~bad])))
    classes, ratios = ur.judge_all(kind, u[adm], mu[adm], var[adm], zeta, ybest)
    occ.add(kind, classes, ratios, var[adm], ur.jones_z(mu[adm], var[adm], zeta, ybest))
    occ.classes[kind]["inadmissible"] += int((~adm).sum())
    worst = float(np.max(ratios)) if len(ratios) else 0.0
    if worst > 1.0:
        w = np.nonzero(adm)[0][int(np.argmax(ratios))]
        print("[%s] %s zeta %g: row %d class %s u %r mu %r var %r ratio %g" %
              (site, kind, zeta, w, classes[int(np.argmax(ratios))], u[w], mu[w], var[w], worst))
    assert worst <= 1.0, (site, kind, zeta, worst, int((ratios > 1.0).sum()))
    want = contract_argmin(u, T)
    assert bi == want, (site, kind, zeta, bi, want)
    if want < 0:
        assert bu == np.inf
    else:
        assert np.float64(bu).view(np.uint64) == u[bi].view(np.uint64)


def calls_of(case, zetas):
    """(kind, zeta, gated): every utility with and without the box / mask gate; Jones from far positive z to underflow."""
    zn, zp = zetas
    return [("agp", 0.01, True), ("agp", 0.01, False), ("bape", 0.01, True), ("bape", 0.01, False),
            ("jones", zn, True), ("jones", zp, False), ("jones", zn, False), ("jones", zp, True),
            ("jones", 1e6, False), ("jones", -50.0, True)]


def run_case(site, case, gp, c, occ):
    """All calls of one case on a computed GP-like object (the device GP, or the oracle stand-in of the CPU dry run)."""
    occ.amp = max(occ.amp, case.amp)
    for kind, zeta, gated in calls_of(case, c["zetas"]):
        box, mask = (c["box"], c["mask"]) if gated else (None, None)
        if case.q:
            idx, ub, u, mu, var = gp.acquire_batch(c["y"], c["T"], kind, case.q, bounds=box, mask=mask, zeta=zeta,
                                                   return_all=True)
            # gp.acquire_batch passes max(y, mu at the earlier picks) as Jones's ybest (the header's rule)
            picks = [int(i) for i in idx[:-1] if i >= 0]
            ybest = max([c["ybest"]] + [float(mu[i]) for i in picks])
            res = (int(idx[-1]), float(ub[-1]), u, mu, var)
            if len(picks) < case.q - 1:
                assert idx[-1] == -1 and ub[-1] == np.inf
                continue
        else:
            res = gp.acquire(c["y"], c["T"], kind, bounds=box, mask=mask, zeta=zeta, return_all=True)
            ybest = c["ybest"]
        check_call(site, kind, zeta, ybest, c["T"], box, mask, res, occ, fantasy=bool(case.q))


@pytest.mark.parametrize("site", sorted(SITES))
def test_utility_epilogue(site):
    from approxposterior_amd import gp as agp
    occ = Occupancy()
    for case in SITES[site]:
        c = build_case(case)
        gp = make_gp(agp, case, c["ell"])
        gp.variance_mode = case.form
        gp.compute(c["X"])
        run_case(site, case, gp, c, occ)
    occ.check(site)


@pytest.mark.parametrize("form", ["inverse", "solve"])
@pytest.mark.parametrize("n,D,m", [(200, 2, 3000), (1100, 3, 5000), (1100, 3, 21384)])
def test_nan_row_never_wins(n, D, m, form):
    """The reference's Jones formula gives a NaN row 0.0 (``sqrt(var) > 0`` is false), and without a box or a mask such
    a row used to pass the gate.  With zeta = 1e6 every other utility is +-0.0 too, so the NaN row at index 0 tied and
    won as the lowest index -- and was handed back as the next design point.  The contract now (include/apgp.h): a row
    with a NaN coordinate is inadmissible, u = +inf, and the winner's coordinates are finite.  Also through the fantasy
    pass."""
    from approxposterior_amd import gp as agp
    case = C(n, D, m, form, 1.0, -20, 1.0, seed=40)
    c = build_case(case)
    T = c["T"]
    T[1, D - 1] = np.nan
    gp = make_gp(agp, case, c["ell"])
    gp.variance_mode = form
    gp.compute(c["X"])
    bi, bu, u, mu, var = gp.acquire(c["y"], T, "jones", zeta=1e6, return_all=True)
    assert np.isposinf(u[0]) and np.isposinf(u[1]) and np.isnan(mu[0]) and np.isnan(var[1])
    assert np.all(u[~nan_rows(T)] == 0.0) and np.all(np.isposinf(u[nan_rows(T)]))
    assert bi >= 0 and np.all(np.isfinite(T[bi])), (bi, T[bi])
    assert bi == 2 and bu == 0.0
    assert gp.acquire(c["y"], T, "jones", zeta=1e6)[0] == 2
    idx, ub = gp.acquire_batch(c["y"], T, "jones", 3, zeta=1e6)
    assert np.all(idx >= 0) and np.all(np.isfinite(T[idx])), (idx, T[idx])
    assert idx[0] == 2
    # all rows NaN: nothing is admissible
    Tn = np.full((130, D), np.nan)
    assert gp.acquire(c["y"], Tn, "jones", zeta=1e6) == (-1, np.inf)
