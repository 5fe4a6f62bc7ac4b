"""GPU: Gaussian-mixture passes whose dynamic LDS exceeds 64 KiB (D = 9..32 with many components), launched with
ascending component counts on one kernel instantiation -- the order fitGMM's BIC loop uses -- in a fresh process,
where the first launch of each instantiation is also the smallest; and the D = 9..16 instantiation against the
NumPy reference."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gmm_ref
from approxposterior_amd import _lib, gmmUtils
from test_gpu_gmm import _abs_stats, _labels_agree, _offset_data, _params, _run

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _check_em(D, K, n, seed):
    import torch
    rs = np.random.RandomState(seed)
    X, centres = _offset_data(rs, n, D, max(K, 2))
    w, c, U = _params(rs, X, K, centres)
    params = gmmUtils._Device(X).pack(w, c, U)
    X_d = torch.from_numpy(X).cuda()
    st, lp, lab = _run(X_d, D, K, params, _lib.GMM_EM)
    ref, rlp, rlab = gmm_ref.em_pass(X, w, c, U)
    np.testing.assert_allclose(lp, rlp, rtol=1e-11)
    assert _labels_agree(lab, rlab, gmm_ref.weighted_log_prob(X, w, c, U))
    _, _, r = gmm_ref.e_step(X, w, c, U)
    scale = np.concatenate([[np.sum(np.abs(rlp))], _abs_stats(X, r, c)])
    assert np.all(np.abs(st - ref) <= 1e-12 * scale + 1e-300)
    sc, _, _ = _run(X_d, D, K, params, _lib.GMM_SCORE, rows=False)
    assert abs(sc[0] - ref[0]) <= 1e-12 * scale[0]
    kc = c + rs.normal(scale=0.5, size=c.shape)
    kst, d2, _ = _run(X_d, D, K, gmmUtils._Device(X).kmeans_pack(kc), _lib.GMM_KMEANS)
    kref, rd2, klab = gmm_ref.kmeans_pass(X, kc)
    np.testing.assert_allclose(d2, rd2, rtol=1e-11)
    onehot = np.zeros((n, K))
    onehot[np.arange(n), klab] = 1.0
    kscale = np.concatenate([[np.sum(rd2)], _abs_stats(X, onehot, kc)])
    assert np.all(np.abs(kst - kref) <= 1e-12 * kscale + 1e-300)


# (D, ascending K): each crosses 64 KiB of dynamic LDS on one instantiation (DP = 32 from K = 7, DP = 16 from K = 10)
ASCENDING = [(20, (6, 7, 16)), (12, (9, 10, 16))]


def ascending_child():
    """run in a fresh process: no earlier launch of these instantiations"""
    for D, ks in ASCENDING:
        for K in ks:
            _check_em(D, K, 3001, 100 * D + K)
    print("ascending OK")


def test_ascending_components_past_64kib_in_a_fresh_process():
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_gmm_lds as t; t.ascending_child()" % (HERE, ROOT))
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ascending OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


@pytest.mark.parametrize("D,K,n", [(12, 9, 257), (16, 16, 100003), (9, 3, 1000), (16, 1, 1)])
def test_d9_to_16_instantiation_against_reference(D, K, n):
    _check_em(D, K, n, 7 * D + K)


def test_fitgmm_bic_loop_up_to_seven_components_at_d20():
    rs = np.random.RandomState(4)
    centres = rs.normal(scale=8.0, size=(3, 20))
    lab = rs.randint(0, 3, size=6000)
    X = centres[lab] + rs.normal(size=(6000, 20))
    g = gmmUtils.fitGMM(X, maxComp=7, gmmKwargs={"random_state": 0})
    assert g.n_components == 3
    np.testing.assert_allclose(g.score(X), gmmUtils._score_on_device(g, X), rtol=1e-10)
