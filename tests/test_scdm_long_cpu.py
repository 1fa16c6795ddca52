"""The long-sentence K1 entry points (tsg_scdm_long_*, more than 32 words) without a GPU: argument checks and the workspace planner
through the built library, the same call list under the host sanitizer build, and the oracle against the reference run captured in
tests/golden/scdm_long.npz (tools/make_golden_scdm_long.py)."""
import os
import sys

import pytest
import torch

from oracle import tsg_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
TOL = dict(atol=2e-6, rtol=1e-5)           # the bound of tests/test_oracle_golden.py


@pytest.fixture(scope="module")
def lib():
    from shufflingvideosfortsg_amd import _lib, build
    build.build()
    return _lib.load()


def test_long_entry_points_reject_bad_arguments_without_gpu(lib):
    """NULL / misaligned pointers, N = 0 and N = NMAX + 1, dtype 7, H = 6, B * T >= 2^31, H / Ds above their limits and a short workspace
    for each of the four entry points; tsg_scdm_long_ws_bytes positive on valid shapes, 0 on rejected ones, no overflow at B = T = 2^30;
    NMAX >= 128; the 32-word entry points still stop at N = 33."""
    import scdm_long_host_driver
    assert scdm_long_host_driver.run_checks(lib) > 150


def test_long_predicates(lib):
    from shufflingvideosfortsg_amd import functional as TF
    assert TF.scdm_long_max_words() >= 128
    assert TF.scdm_long_ok(48, 1024, 1024) and TF.scdm_long_ok(1, 4, 4) and TF.scdm_long_ok(TF.scdm_long_max_words(), 260, 516)
    assert not TF.scdm_long_ok(TF.scdm_long_max_words() + 1, 64, 64)
    assert not TF.scdm_long_ok(48, 1028, 64) and not TF.scdm_long_ok(48, 64, 1028) and not TF.scdm_long_ok(48, 6, 64)


def test_long_functions_have_no_cpu_fallback(lib):
    from shufflingvideosfortsg_amd import functional as TF
    a = torch.randn(1, 4, 8); s = torch.randn(1, 40, 8); w = torch.randn(8); v = torch.randn(1, 40, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TF.scdm_attn_long(a, s, w, v)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TF.scdm_gate_long(a, s, w, v, torch.randn(8), torch.randn(1, 4, 8))


def test_long_host_layer_under_address_and_ub_sanitizers():
    """The same call list through the AddressSanitizer + UndefinedBehaviorSanitizer build of the host layer (tools/build_host_sanitized.py
    compiles every csrc/*.hip host-only, scdm_long.hip included).  CPU only: nothing is launched."""
    import subprocess
    tool = os.path.join(ROOT, "tools", "build_host_sanitized.py")
    if not os.path.exists(tool):
        pytest.skip("tools/build_host_sanitized.py is not here")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import build_host_sanitized as san_build
    try:
        rt = san_build.asan_runtime()
    except Exception as e:                     # no ASAN runtime on this machine
        pytest.skip(f"no AddressSanitizer runtime: {e}")
    if not rt or not os.path.exists(rt):
        pytest.skip("no AddressSanitizer runtime")
    san = san_build.build_sanitized()
    env = dict(os.environ, LD_PRELOAD=rt, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "scdm_long_host_driver.py"), san], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "long-sentence host-side calls clean" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


@pytest.mark.parametrize("tag", ["n40", "n48"])
def test_oracle_reproduces_the_reference_at_long_sentences(golden, tag):
    """oracle.scdm_attention / recalibration_layer against the real reference's SCDM_Attention and rnn_recalibration_layer at N = 40 and 48."""
    g = golden("scdm_long")
    w = {k: v.clone().requires_grad_(True) for k, v in g.group(f"{tag}.att.w.").items()}
    v = g.t(f"{tag}.video").requires_grad_(True); s = g.t(f"{tag}.sent").requires_grad_(True)
    assert s.shape[1] == int(tag[1:]) > 32
    C = O.scdm_attention(v, s, w["W_s.weight"], w["W_a.weight"], w["W_a.bias"], w["w.weight"])
    torch.testing.assert_close(C, g.t(f"{tag}.C"), **TOL)
    C.backward(g.t(f"{tag}.gC"))
    torch.testing.assert_close(v.grad, g.t(f"{tag}.gvideo"), **TOL)
    torch.testing.assert_close(s.grad, g.t(f"{tag}.gsent"), **TOL)
    for k, want in g.group(f"{tag}.att.gw.").items():
        torch.testing.assert_close(w[k].grad, want, **TOL, msg=lambda m, k=k: f"{k}: {m}")
    p = {k: t.clone().requires_grad_(True) for k, t in g.group(f"{tag}.rec.w.").items()}
    rv = g.t(f"{tag}.rec.video").requires_grad_(True); rw = g.t(f"{tag}.rec.word").requires_grad_(True)
    out = O.recalibration_layer(rv, rw, p)
    torch.testing.assert_close(out, g.t(f"{tag}.rec.out"), **TOL)
    out.backward(g.t(f"{tag}.rec.g"))
    torch.testing.assert_close(rv.grad, g.t(f"{tag}.rec.gvideo"), **TOL)
    torch.testing.assert_close(rw.grad, g.t(f"{tag}.rec.gword"), **TOL)
    for k, want in g.group(f"{tag}.rec.gw.").items():
        torch.testing.assert_close(p[k].grad, want, **TOL, msg=lambda m, k=k: f"{k}: {m}")
