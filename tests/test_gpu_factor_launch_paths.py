"""GPU: the host side of the factorisation's launch paths in the order that exposes shared set-up -- in ONE fresh
process, where every once-per-device LDS flag starts unset and the stream's scratch does not exist yet:
  1. apgp_nll_eval at n = 100 (nll_two_kernel), then at D = 5: another instantiation, which raises its own LDS limit;
  2. n = 130 (three block columns): the persistent launch;
  3. apgp_nll_eval_batch, n = 130, B = 2, side by side: the slot-2 scratch regrows right after a single call;
  4. the single call again;  5. B = 3;  6. n = 100, B = 3 (nll_two_kernel's batched instantiation);
  7. n = 130 in mode 2 (the persistent launch gives up, the evaluation runs again) and in mode 1 (a launch per step).
What must hold: every status 0; the counters of side-by-side batches and of fallbacks move exactly as the steps say;
factor, z and record of one matrix are the same bits on every path and in every batch; the factor meets the Cholesky
bar of factor_ref.py.  (A limit never raised for a second kernel fails its launch; a field the argument builder leaves
out, or scratch shared wrongly between the single and the batched launch, changes bits or hangs the child, which runs
under its own time limit.)"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import factor_ref as fr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
N3, N2, B_MAX = 130, 100, 3          # three block columns | two | the largest batch
CHILD_SECONDS = 120


def _inputs():
    rs = np.random.RandomState(20261)
    X = rs.uniform(-5, 5, size=(N3, 2))
    y = np.sin(X[:, 0]) + 0.3 * X[:, 1] ** 2
    X5 = rs.uniform(-5, 5, size=(N2, 5))
    metrics = [np.array([8.0, 8.0]), np.array([5.0, 11.0]), np.array([9.5, 4.5])]
    means = np.array([float(np.median(y)) + 0.1 * b for b in range(B_MAX)])
    return X, y, X5, metrics, means


def launch_paths_child(path):
    """run in a fresh process; writes what it saw to ``path`` (.npz)"""
    import torch
    from approxposterior_amd import _lib
    from approxposterior_amd import gp as agp
    lib = _lib.load()
    X, y, X5, metrics, means = _inputs()

    def kstruct(metric):
        g = agp.GP(kernel=agp.ExpSquaredKernel(metric, ndim=len(metric)), fit_mean=True, mean=0.0, white_noise=-12,
                   fit_white_noise=False)
        g._yerr2 = 0.0
        return g._kernel_struct()

    ks = [kstruct(m) for m in metrics]
    karr = (_lib.KernelStruct * B_MAX)(*ks)
    Xd, X5d, yd = torch.from_numpy(X).cuda(), torch.from_numpy(X5).cuda(), torch.from_numpy(y).cuda()
    X100d = torch.from_numpy(np.ascontiguousarray(X[:N2])).cuda()
    out, tags = {}, []

    def counters():
        return np.array([lib.apgp_nll_side_batches(), lib.apgp_potrf_fallbacks()])

    def single(tag, Xdev, n, k, mean):
        K = torch.zeros((n, n), dtype=torch.float64, device="cuda")
        z = torch.empty(n, dtype=torch.float64, device="cuda")
        info = torch.empty(1, dtype=torch.int32, device="cuda")
        o5 = torch.empty(5, dtype=torch.float64, device="cuda")
        o = np.full(5, np.nan)
        rc = lib.apgp_nll_eval(Xdev.data_ptr(), n, ctypes.byref(k), yd.data_ptr(), mean, K.data_ptr(), z.data_ptr(),
                               info.data_ptr(), o5.data_ptr(), o.ctypes.data, None)
        torch.cuda.synchronize()
        assert rc == 0, (tag, rc, lib.apgp_last_error())          # (and nothing more is launched)
        tags.append(tag)
        out[tag + "_L"], out[tag + "_z"], out[tag + "_rec"] = torch.tril(K).cpu().numpy(), z.cpu().numpy(), o
        out[tag + "_rec_dev"], out[tag + "_info"] = o5.cpu().numpy(), info.cpu().numpy()
        out[tag + "_count"] = counters()

    def batch(tag, Xdev, n, B):
        K = torch.zeros((B, n, n), dtype=torch.float64, device="cuda")
        z = torch.empty((B, n), dtype=torch.float64, device="cuda")
        info = torch.empty(B, dtype=torch.int32, device="cuda")
        o5 = torch.empty((B, 5), dtype=torch.float64, device="cuda")
        o = np.full((B, 5), np.nan)
        rc = lib.apgp_nll_eval_batch(Xdev.data_ptr(), n, B, ctypes.addressof(karr), yd.data_ptr(), means.ctypes.data,
                                     K.data_ptr(), z.data_ptr(), info.data_ptr(), o5.data_ptr(), o.ctypes.data, None)
        torch.cuda.synchronize()
        assert rc == 0, (tag, rc, lib.apgp_last_error())          # (and nothing more is launched)
        tags.append(tag)
        out[tag + "_L"], out[tag + "_z"], out[tag + "_rec"] = torch.tril(K).cpu().numpy(), z.cpu().numpy(), o
        out[tag + "_rec_dev"], out[tag + "_info"] = o5.cpu().numpy(), info.cpu().numpy()
        out[tag + "_count"] = counters()

    k5 = kstruct(np.array([8.0, 6.0, 10.0, 7.0, 9.0]))
    lib.apgp_potrf_mode(0)
    out["start_count"] = counters()
    single("s1_two", X100d, N2, ks[0], means[0])
    single("s1_two_d5", X5d, N2, k5, means[0])
    single("s2_single", Xd, N3, ks[0], means[0])
    batch("s3_batch2", Xd, N3, 2)
    single("s4_single", Xd, N3, ks[0], means[0])
    batch("s5_batch3", Xd, N3, 3)
    batch("s6_two_batch3", X100d, N2, 3)
    lib.apgp_potrf_mode(2)
    single("s7_give_up", Xd, N3, ks[0], means[0])
    lib.apgp_potrf_mode(1)
    single("s7_steps", Xd, N3, ks[0], means[0])
    lib.apgp_potrf_mode(0)
    # (after the steps under test) the other matrices of the batches as single calls, and the Gram matrix's bits
    for b in (1, 2):
        single("after_single_%d" % b, Xd, N3, ks[b], means[b])
        single("after_two_%d" % b, X100d, N2, ks[b], means[b])
    G = torch.zeros((N3, N3), dtype=torch.float64, device="cuda")
    rc = lib.apgp_gram(Xd.data_ptr(), N3, ctypes.byref(ks[0]), G.data_ptr(), N3, None)
    torch.cuda.synchronize()
    assert rc == 0, ("apgp_gram", rc, lib.apgp_last_error())
    out["gram"] = G.cpu().numpy()
    out["cus"] = np.array(torch.cuda.get_device_properties(0).multi_processor_count)
    out["tags"] = np.array(tags)
    np.savez(path, **out)
    print("launch paths OK")


@pytest.fixture(scope="module")
def seen(tmp_path_factory):
    """the child's record: one run shared by the tests below, which only read it"""
    path = str(tmp_path_factory.mktemp("factor_launch_paths") / "seen.npz")
    code = ("import sys; sys.path[:0] = [%r, %r, %r]; import test_gpu_factor_launch_paths as t; t.launch_paths_child(%r)"
            % (HERE, ROOT, os.path.join(ROOT, "oracle"), path))
    proc = subprocess.run(["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, "-c", code], cwd=ROOT,
                          capture_output=True, text=True)
    # (nothing more is started on the device after a child that failed, faulted or ran into its limit)
    assert proc.returncode == 0 and "launch paths OK" in proc.stdout, \
        "child exit status %d\n%s\n%s" % (proc.returncode, proc.stdout[-2000:], proc.stderr[-4000:])
    with np.load(path) as f:
        return {k: f[k] for k in f.files}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


STEPS = ["s1_two", "s1_two_d5", "s2_single", "s3_batch2", "s4_single", "s5_batch3", "s6_two_batch3", "s7_give_up", "s7_steps"]


def test_every_call_succeeds_and_factorises(seen):
    assert list(seen["tags"][:len(STEPS)]) == STEPS              # (the child stops at the first status that is not 0)
    for tag in seen["tags"]:
        assert not np.any(seen[tag + "_info"]), tag
        assert np.all(seen[tag + "_rec"][..., 4] == 0.0), (tag, seen[tag + "_rec"])
        assert same_bits(seen[tag + "_rec"], seen[tag + "_rec_dev"]), tag        # (the host's record is the device's)
        assert np.all(np.isfinite(seen[tag + "_L"])) and np.all(np.isfinite(seen[tag + "_z"])), tag


def test_fallback_counter_moves_in_the_give_up_step_only(seen):
    fallbacks = [int(seen["start_count"][1])] + [int(seen[t + "_count"][1]) for t in STEPS]
    assert fallbacks[:8] == [fallbacks[0]] * 8, fallbacks             # start, steps 1 .. 6: nothing
    assert fallbacks[8] == fallbacks[0] + 1, fallbacks                # step 7, mode 2: exactly one
    assert fallbacks[9] == fallbacks[8], fallbacks                    # step 7, mode 1: none


def test_side_by_side_counter_moves_in_steps_3_and_5(seen):
    cus, nb = int(seen["cus"]), (N3 + 63) // 64
    if cus < B_MAX * (nb + 2):
        pytest.skip("side by side needs B (nb + 2) = %d compute units, the device has %d" % (B_MAX * (nb + 2), cus))
    side = [int(seen["start_count"][0])] + [int(seen[t + "_count"][0]) for t in STEPS]
    assert [b - a for a, b in zip(side, side[1:])] == [0, 0, 0, 1, 0, 1, 0, 0, 0], side


@pytest.mark.parametrize("tag", ["s4_single", "s7_give_up", "s7_steps"])
def test_one_matrix_same_bits_on_every_path(seen, tag):
    for what in ("_L", "_z", "_rec"):
        assert same_bits(seen[tag + what], seen["s2_single" + what]), (tag, what)


@pytest.mark.parametrize("tag,B,first", [("s3_batch2", 2, "s2_single"), ("s5_batch3", 3, "s2_single"),
                                         ("s6_two_batch3", 3, "s1_two")])
def test_batches_equal_the_single_calls(seen, tag, B, first):
    after = "after_single_%d" if first == "s2_single" else "after_two_%d"
    for b in range(B):
        one = first if b == 0 else after % b
        for what in ("_rec", "_L", "_z"):
            assert same_bits(seen[tag + what][b], seen[one + what]), (tag, b, what)
    # (the matrices of a batch differ: one matrix's result under every index would not pass)
    assert not same_bits(seen[tag + "_rec"][0], seen[tag + "_rec"][1])


def test_factor_meets_the_cholesky_bar(seen):
    r = fr.chol_ratio(seen["gram"], seen["s2_single_L"]).max()
    print("n = %d: worst |A - L L^T| / budget %.3f" % (N3, r))
    assert r <= 1.0
