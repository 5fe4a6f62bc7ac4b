# -*- coding: utf-8 -*-
"""The error budget of the bf16 matrix-core coarse bound (csrc/prune_mm32.h, "Error of mu32"), on the CPU: the NumPy
replay of tests/prune_mmbf16_ref.py against the exact values.

* the split: h + m + l = p exactly, every part a bf16 number, |m| <= 2^-8 |p|, |l| <= 2^-17 |p|, over 10^6 fp32 values
  (both signs, magnitudes from 2^-100 to 2^50, the gate's range) and over powers of two and full mantissas;
* the k slots: every kept product once, the small ones first in ascending order, the big ones in the last instruction;
* the exponent within eta0 of the truth under the measured model of the instruction AND under one rounding to nearest or
  one truncation per addend, and |mu32 - mu| <= e32: a candidate on a training point, A >> B, B >> A, one dominant
  coordinate, inputs at the gate's edge; D = 1, 3, 8;
* the existing two-sided GPU tests (test_gpu_prune_mm32.test_row_mapping, test_gpu_prune_mm32_pipeline) keep holding:
  on their shapes the emulated device bound lies in [b - 2 slack_old, b];
* tests/test_gpu_prune_mmbf16.py can see a fault: for each mutated replay its two-sided check fails on its own
  one-coordinate inputs."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import prune_mm32_ref as mm                      # noqa: E402
import prune_mmbf16_ref as bf                    # noqa: E402
import prune_ref as pr                           # noqa: E402
import util_ref                                  # noqa: E402

F = np.float32
MODES = ["model", "rne", "rz"]


def _alpha(X, y, metric, D):
    import bench
    gpo, _ = bench.oracle_gp(X, y, metric, D)
    return np.asarray(gpo._alpha if hasattr(gpo, "_alpha") else gpo.alpha, dtype=np.float64).ravel()


def test_split_is_exact():
    rs = np.random.RandomState(3)
    n = 10 ** 6
    p = (rs.uniform(1.0, 2.0, n) * rs.choice([-1.0, 1.0], n) * np.exp2(rs.randint(-100, 51, n))).astype(F)
    e = np.arange(-100, 51)
    special = np.concatenate([np.exp2(e), -np.exp2(e), np.exp2(e) * (2.0 - 2.0 ** -23), -np.exp2(e) * (2.0 - 2.0 ** -23),
                              np.exp2(e) * (1.0 + 2.0 ** -23), np.exp2(e) * (1.0 + 2.0 ** -8 + 2.0 ** -16), [0.0, -0.0]]).astype(F)
    for v in (p, special):
        h, m, l = bf.split(v)
        d = np.float64
        assert np.all(h.astype(d) + m.astype(d) + l.astype(d) == v.astype(d))
        for part in (h, m, l):
            assert np.all(bf.bf16(part) == part)
        assert np.all(np.abs(m) <= 2.0 ** -8 * np.abs(v)) and np.all(np.abs(l) <= 2.0 ** -17 * np.abs(v))
    # the "1" of both sides has an h part only
    h, m, l = bf.split(np.ones(1, dtype=F))
    assert h[0] == 1.0 and m[0] == 0.0 and l[0] == 0.0


@pytest.mark.parametrize("dpad,nis", [(2, 1), (4, 2), (8, 3)])
def test_slots(dpad, nis):
    sl = bf.slots(dpad)
    K = dpad + 2
    assert bf.counts(dpad) == (nis, nis + 1) and len(sl) == 16 * (nis + 1)
    kept = [s for s in sl if s[0] >= 0]
    assert len(kept) == len(set(kept)) == 6 * dpad + 6
    want = {(e, 0, 0) for e in range(K)} | {(0, 1, 0), (0, 2, 0), (1, 0, 1), (1, 0, 2)}
    want |= {(2 + d, pp, qp) for d in range(dpad) for pp, qp in ((0, 1), (1, 0), (1, 1), (0, 2), (2, 0))}
    assert set(kept) == want
    # the big products fill the last instruction's first K slots, in entry order; no big product before it
    assert sl[16 * nis:16 * nis + K] == [(e, 0, 0) for e in range(K)]
    assert all(s[0] < 0 or (s[1], s[2]) != (0, 0) for s in sl[:16 * nis])
    # lowest order first: the sum of the two parts' orders (h 0, m 8, l 17 bits down) does not increase
    down = {0: 0, 1: 8, 2: 17}
    order = [down[s[1]] + down[s[2]] for s in sl[:16 * nis] if s[0] >= 0]
    assert order == sorted(order, reverse=True)


def _shaped_inputs(name, D, n=40, m=60):
    """(X, T, metric): synthetic training rows and candidates in [-5, 5]^D shaped for one edge of the budget."""
    rs = np.random.RandomState(7 + D)
    X = rs.uniform(-5.0, 5.0, size=(n, D))
    T = rs.uniform(-5.0, 5.0, size=(m, D))
    metric = np.full(D, 8.0)
    if name == "on a training point":
        T[:n // 2] = X[:n // 2]
    elif name == "A >> B":
        X = X[0] + 1e-3 * (X - X[0])
    elif name == "B >> A":
        T = X[0] + 1e-3 * (T - X[0])
    elif name == "one dominant coordinate":
        X[:, 1:] = X[0, 1:] + 1e-4 * (X[:, 1:] - X[0, 1:])
        T[:, 1:] = X[0, 1:] + 1e-4 * (T[:, 1:] - X[0, 1:])
    elif name == "gate's edge":
        # scale the metric until the largest eta sits just inside 2^-8
        sc = np.sqrt(0.5 / metric)
        c = X[0] * sc
        A = np.sqrt((((T * sc) - c) ** 2).sum(axis=1)).max()
        B = np.sqrt((((X * sc) - c) ** 2).sum(axis=1)).max()
        f = np.sqrt((2.0 ** -8 - 24.0 * bf.U32) / ((bf.dpad_of(D) + 10.0) * bf.U32 * (A + B) ** 2)) * (1.0 - 1e-6)
        metric = metric / f ** 2
    else:
        raise ValueError(name)
    return X, T, metric


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["on a training point", "A >> B", "B >> A", "one dominant coordinate", "gate's edge"])
@pytest.mark.parametrize("D", [1, 3, 8])
def test_exponent_within_eta0(D, name, mode):
    X, T, metric = _shaped_inputs(name, D)
    rs = np.random.RandomState(11)
    alpha = rs.standard_normal(len(X)) * np.exp(rs.uniform(-3.0, 3.0, len(X)))
    r = bf.replay(X, alpha, T, np.sqrt(0.5 / metric), mode=mode)
    ok = r["gate"]
    print("[D=%d %s, %s] A <= %.3g, B = %.3g, eta <= %.3g, gate passes for %d of %d; exponent error / eta0 <= %.3g; "
          "|mu32 - mu| / e32 <= %.3g" % (D, name, mode, r["A"].max(), r["B"], r["eta"].max(), int(ok.sum()), len(ok),
                                         (r["exp_err"] / r["eta0"]).max(), (np.abs(r["mu32"] - r["mu"])[ok] / r["e32"][ok]).max()))
    assert ok.all()
    if name == "gate's edge":
        assert r["eta"].max() > 0.99 * 2.0 ** -8
    assert np.all(r["exp_err"] <= r["eta0"])
    assert np.all(np.abs(r["mu32"] - r["mu"]) <= r["e32"])
    # S32 bounds the exact sum of |alpha| k from above within the same budget (the flushed values: the absolute term)
    assert np.all(r["S"] <= r["S32"] * np.exp(r["eta"]) + 2.0 ** -120 * (r["sa"] + r["n"]))
    assert np.all(r["khat_max"] <= np.exp(r["eta"]) * (1.0 + 4.0 * bf.U32))


def _two_sided(kind, r, sl, mu32, mean, ybest, n):
    """(device bound as the replay has it, b): the GPU tests assert b - 2 slack <= bound <= b."""
    mu = r["mu"] + mean
    one = np.ones(len(mu))
    b = pr.row_bounds(kind, mu, 1.0, r["S"], np.ones(len(mu), dtype=bool), n, r["dpad"], 0.01, ybest)
    got = util_ref.f64(kind, mu32 + mean, one, 0.01, ybest) - sl
    return got, b


# the shapes of test_gpu_prune_mm32.test_row_mapping, and of test_gpu_prune_mm32_pipeline at its largest n per width
@pytest.mark.parametrize("n,D,m", [(33, 2, 576), (130, 2, 576), (513, 3, 576), (130, 8, 576), (257, 1, 513), (257, 8, 513),
                                   (33, 1, 513), (129, 8, 513)])
def test_existing_two_sided_tests_keep_holding(n, D, m):
    import bench
    X, y = bench.synthetic_c3(n, D)
    T = np.random.RandomState(1).uniform(-5.0, 5.0, size=(m, D))
    T[m // 2] = X[min(7, n - 1)]
    alpha = _alpha(X, y, 8.0, D)
    sc = np.sqrt(0.5 / np.full(D, 8.0))
    mean, ybest = float(np.median(y)), float(np.max(y))
    rows = np.concatenate([np.arange((m + 63) // 64) * 64 + kept for kept in (0, 31, 32, 63)])
    rows = rows[rows < m]
    new = bf.replay(X, alpha, T[rows], sc)
    old = mm.replay(X, alpha, T[rows], sc)
    assert new["gate"].all() and old["gate"].all()
    worst = 0.0
    for kind in util_ref.KINDS:
        b0 = util_ref.f64(kind, new["mu"] + mean, np.ones(len(rows)), 0.01, ybest)
        sl_new = bf.slack(kind, b0, new["mu"] + mean, 1.0, new, 0.01, ybest)
        sl_old = mm.slack(kind, b0, old["mu"] + mean, 1.0, old, 0.01, ybest)
        got, b = _two_sided(kind, new, sl_new, new["mu32"], mean, ybest, n)
        worst = max(worst, ((b - got) / sl_old).max(), (sl_new / sl_old).max())
        assert np.all(got <= b) and np.all(b - 2.0 * sl_old <= got), (kind, got, b, sl_old)
    print("[n=%d D=%d] (b - emulated bound) / slack_old and slack_new / slack_old <= %.3f (the tests allow 2)" % (n, D, worst))


def mutations(dpad, d):
    """The faults of the issue's list, for a set that differs in coordinate d alone."""
    nis = bf.counts(dpad)[0]
    big = 16 * nis
    return ([("drop", k) for k in ("hh", "hm", "mh", "mm", "hl", "lh")] +
            [("swap", 2 * d, 2 * d + 1),                                 # h l and l h of the coordinate
             ("swap", big, big + 1),                                     # the two norm entries
             ("swap", big + 2 + d, big + 2 + (d + 1) % dpad),            # two coordinates' big products
             ("swap", 2 * dpad + 2 + d, big + 2 + d)] +                  # across two instructions: m m and h h
            [("zero", side, part) for side in ("P", "Q") for part in (1, 2)])


@pytest.mark.parametrize("D", [1, 2, 3, 8])
def test_the_gpu_check_sees_each_fault(D):
    dpad = bf.dpad_of(D)
    sc = np.sqrt(0.5 / np.full(D, bf.ONE_METRIC))
    for d in range(D):
        X, y, T = bf.one_coordinate_case(D, d)
        assert np.all(np.abs(X) <= 5.0) and np.all(np.abs(T) <= 5.0)
        alpha = _alpha(X, y, bf.ONE_METRIC, D)
        mean, ybest = float(np.median(y)), float(np.max(y))
        r = bf.replay(X, alpha, T, sc)
        assert r["gate"].all()
        sls = {}
        for kind in util_ref.KINDS:
            b0 = util_ref.f64(kind, r["mu"] + mean, np.ones(len(T)), 0.01, ybest)
            sls[kind] = bf.slack(kind, b0, r["mu"] + mean, 1.0, r, 0.01, ybest)
            got, b = _two_sided(kind, r, sls[kind], r["mu32"], mean, ybest, len(X))
            assert np.all(got <= b) and np.all(b - 2.0 * sls[kind] <= got), (D, d, kind)
        for mut in mutations(dpad, d):
            bad = bf.replay(X, alpha, T, sc, mutate=mut)
            seen = 0
            for kind in util_ref.KINDS:
                got, b = _two_sided(kind, r, sls[kind], bad["mu32"], mean, ybest, len(X))
                seen += int(np.sum(~((got <= b) & (b - 2.0 * sls[kind] <= got))))
            assert seen > 0, (D, d, mut)
