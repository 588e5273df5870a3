"""CPU-side checks of the cloud resampling: the NumPy restatement against the oracle's generator and a C truncation, the host-callable rules
of glim_amd/csrc/resample.hpp run from a stand-alone program (plain and under the address / undefined-behaviour sanitizers), the C++ mirror
compiling and linking, the declared symbols, and the argument checks that need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import resample_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _below_target_pairs(limit=12):
    """(n, target) for which n * (target / n) lands just below target in FP64: the truncation then keeps target - 1 points, as
    `frame->size() * sampling_rate` does upstream"""
    out = []
    for n in range(2, 600):
        for t in range(1, n):
            if float(n) * (float(t) / float(n)) < float(t):
                out.append((n, t))
                if len(out) >= limit:
                    return out
    return out


def test_the_restated_hash_is_the_oracles(orc):
    L = orc.lib()
    rng = np.random.default_rng(0)
    pairs = [(0, 0), (R.sample_hash.__globals__["MASK"], 5), (7, (1 << 32) + 3)]
    pairs += [(int(s), int(i)) for s, i in zip(rng.integers(0, 1 << 63, size=3000, dtype=np.uint64), rng.integers(0, 1 << 40, size=3000))]
    for seed, index in pairs:
        assert R.sample_hash(seed, index) == L.orc_sample_hash(seed, index), (seed, index)
    k = R.keys(100, 7)
    assert k.dtype == np.uint32 and [int(v) for v in k] == [L.orc_sample_hash(7, i) >> 32 for i in range(100)]


def test_count_is_the_truncation_of_a_c_double_product():
    pairs = _below_target_pairs()
    assert len(pairs) >= 4
    cases = [(1000, 0.1), (1000, 0.5), (1000, 0.98), (1000, 0.0), (1000, 1e-9), (7, 0.5), (0, 0.5), (1 << 28, 0.3)]
    cases += [(n, float(t) / float(n)) for n, t in pairs]
    for n, rate in cases:
        want = int(C.c_int64(int(C.c_double(C.c_double(float(n)).value * C.c_double(rate).value).value)).value)
        assert R.count(n, rate) == want, (n, rate)
    for n, t in pairs:
        if float(t) / float(n) < R.FULL_RATE:
            assert R.count(n, float(t) / float(n)) == t - 1, (n, t)
    # from 0.99 on: the whole cloud
    assert R.count(1000, 0.99) == 1000 and R.count(1000, 1.0) == 1000 and R.count(1000, 3.0) == 1000 and R.count(1000, 0.9899) == 989


def test_selection_and_indices_of_the_restatement_agree_with_a_plain_sort():
    rng = np.random.default_rng(1)
    for n, m in ((1, 1), (10, 0), (10, 10), (257, 100), (1000, 999)):
        k = rng.integers(0, 4, size=n).astype(np.uint32)  # dense ties
        want = sorted(sorted(range(n), key=lambda i: (int(k[i]), i))[:m])
        np.testing.assert_array_equal(np.nonzero(R.select_smallest(k, m))[0], want)
    idx = R.random_sample_indices(1000, 0.1, 3)
    k = R.keys(1000, 3)
    want = sorted(sorted(range(1000), key=lambda i: (int(k[i]), i))[:100])
    np.testing.assert_array_equal(idx, want)
    np.testing.assert_array_equal(R.random_sample_indices(50, 0.99, 3), np.arange(50))
    assert len(R.random_sample_indices(50, 0.0, 3)) == 0


# ---- the host-callable rules of resample.hpp, from a stand-alone program ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("resample_host")
    src = os.path.join(ROOT, "tests", "cpp", "test_resample_host.cpp")
    out = {}
    for name, flags in (("plain", ["-O2"]), ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(d / name)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", *flags, src, "-o", exe])
        out[name] = exe
    return out


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_rules_on_the_host_equal_the_restatement(host_programs, tmp_path, build):
    rng = np.random.default_rng(2)
    seed, num_keys, n = 0x9E3779B97F4A7C15, 2000, 40
    counts = [(1000, 0.1), (1000, 0.5), (4097, 0.98), (5, 0.0), (123456789, 1e-9), (1000, 0.99), (10, 3.0)]
    counts += [(a, float(t) / float(a)) for a, t in _below_target_pairs()]
    # a pose with a translation of order 20 m, and a linear part that is no rotation
    c, s = np.cos(0.7), np.sin(0.7)
    rigid = np.array([[c, -s, 0.0, 21.5], [s, c, 0.0, -19.25], [0.0, 0.0, 1.0, 3.125]])
    shear = np.array([[1.5, 0.25, -0.125, 1.0], [0.0, -2.0, 0.5, -3.0], [0.75, 0.0, 0.3, 20.0]])
    p = np.concatenate([rng.uniform(-30.0, 30.0, size=(n, 3)), np.ones((n, 1))], axis=1)
    p[1, 3] = 0.0
    p[2, 0], p[3, 1] = np.nan, np.inf
    a = rng.normal(size=(n, 3, 3))
    c6 = R.cov6(a @ np.transpose(a, (0, 2, 1)))
    nr = rng.normal(size=(n, 3))
    for T in (rigid, shear, np.eye(4)[:3]):
        inp, outp = str(tmp_path / "in.txt"), str(tmp_path / "out.txt")
        with open(inp, "w") as f:
            f.write(f"{seed} {num_keys}\n{len(counts)}\n")
            for cn, rate in counts:
                f.write(f"{cn} {float(rate).hex()}\n")
            f.write(" ".join(float(v).hex() for v in T.reshape(12)) + f"\n{n}\n")
            for row in np.concatenate([p, c6, nr], axis=1):
                f.write(" ".join(float(v).hex() for v in row) + "\n")
        out = subprocess.run([host_programs[build], inp, outp], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        lines = open(outp).read().splitlines()
        np.testing.assert_array_equal(np.array(lines[0].split(), dtype=np.uint64), R.keys(num_keys, seed).astype(np.uint64))
        assert [int(v) for v in lines[1].split()] == [R.count(cn, rate) for cn, rate in counts]
        got = np.array([line.split() for line in lines[2:]], dtype=np.uint64)
        q, d, m = R.transform(p, c6, nr, T)
        want = np.concatenate([q, d, m], axis=1)
        # NaN payloads are not part of the rule: a NaN must be a NaN, everything else the same bits
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got.view(np.float64)), nan) and nan.any()
        np.testing.assert_array_equal(got[~nan], want.view(np.uint64)[~nan])
    print(build, "rows compared:", n, "counts:", len(counts))


# ---- the C++ mirror, and the C ABI without a device ------------------------------------------------------------------------------------------------
def test_cpp_mirror_compiles_links_and_throws_on_a_refused_call(tmp_path):
    from glim_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exe = str(tmp_path / "test_resample_mirror")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_resample_mirror.cpp"), "-o", exe, "-L" + os.path.join(ROOT, "glim_amd"), "-lglim_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "glim_amd"), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "resample mirror: ok" in out.stdout


def test_symbols_are_declared_and_the_python_api_names_exist():
    from glim_amd import _lib, api

    for name in ("glim_amd_cloud_random_sample", "glim_amd_cloud_sample", "glim_amd_cloud_transform", "glim_amd_debug_select_smallest"):
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name)
    for name in ("random_sampling", "sample", "transform"):
        assert callable(getattr(api.PointCloudGPU, name))
    assert callable(api.debug_select_smallest)
    stable = open(os.path.join(ROOT, "include", "glim_amd.h")).read()
    diag = open(os.path.join(ROOT, "include", "glim_amd_diag.h")).read()
    assert "glim_amd_debug_select_smallest(" in diag and "glim_amd_debug_select_smallest" not in stable
    assert "as recalled" in stable.lower()  # the 0.99 shortcut is a recollection, and the header says so


def test_argument_errors_return_the_stated_codes_without_a_device():
    from glim_amd import _lib

    L = _lib.lib()
    INVALID = -1
    h = C.c_void_p()
    T = np.eye(4)[:3].reshape(12).copy()
    dp = T.ctypes.data_as(C.POINTER(C.c_double))
    idx = np.zeros(4, dtype=np.int32)
    ip = idx.ctypes.data_as(C.POINTER(C.c_int32))
    keys = np.zeros(4, dtype=np.uint32)
    kp = keys.ctypes.data_as(C.POINTER(C.c_uint32))
    for rate in (0.5, float("nan"), float("inf"), -0.1):
        assert L.glim_amd_cloud_random_sample(None, rate, 0, C.byref(h)) == INVALID
    assert L.glim_amd_cloud_sample(None, 4, ip, C.byref(h)) == INVALID
    assert L.glim_amd_cloud_sample(None, 0, None, C.byref(h)) == INVALID
    assert L.glim_amd_cloud_transform(None, dp, C.byref(h)) == INVALID
    assert not h.value
    assert L.glim_amd_debug_select_smallest(None, 4, kp, 2, ip) == INVALID
