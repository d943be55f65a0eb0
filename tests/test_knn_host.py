"""CPU: the host side of the binning-free mutual-information scores -- the restatement tests/knn_ref.py against the installed
scikit-learn's _compute_mi_cd BIT FOR BIT, digamma_integers against scipy, the scores from hand-made matrices, the fourteenth
library's C-ABI (include/dvae_knn_hip.h == disvae_amd/_knnlib.py == the built lib_scores/libdvae_knn_hip.so), its row of build.py's
SCORE_TARGETS (asserted to be IN the list and IN the directory, never to be all of either: the next score library is one more
row there), the LDS plan of the header against 160 KiB, the rules its source obeys, the refusal of bad arguments before any launch
and the argument errors of the public functions before any device work.

mutual_info_classif itself is not the reference: it rescales the column and adds seeded noise of 1e-10; the estimator here adds
none and handles ties by its own rule, which is _compute_mi_cd's.
"""
import ctypes
import importlib.util
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import knn_ref as R
import disvae_amd
from disvae_amd import _cabi, _infolib, _knnlib, _lib, _saplib
from disvae_amd import evaluate as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dvae_knn_hip.h")
CSRC = os.path.join(ROOT, "disentangling-vae_amd", "csrc")
SOURCE = "knn_mi.hip"
DUMMY = 1 << 20                                                   # aligned non-NULL address, never dereferenced


def _build():
    spec = importlib.util.spec_from_file_location("dvae_build_knn", os.path.join(ROOT, "disentangling-vae_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _nm(path, *flags):
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin")
    assert nm, "no nm on this machine"
    return subprocess.run([nm] + list(flags) + [path], capture_output=True, text=True, check=True).stdout


# ---- 1. the restatement against scikit-learn --------------------------------------------------------------------------------------
def _scipy_psi(n):
    special = pytest.importorskip("scipy.special")
    return np.concatenate([[0.0], special.digamma(np.arange(1, n + 1))])


def _columns(S, seed):
    rng = np.random.default_rng(seed)
    centre = rng.integers(0, 3, S) * 1.5
    cont = (centre + 0.4 * rng.standard_normal(S)).astype(np.float32)
    return {"continuous": cont, "rounded-1/64": (np.round(cont * 64.0) / 64.0).astype(np.float32),
            "constant": np.full(S, 0.75, dtype=np.float32), "two-valued": rng.integers(0, 2, S).astype(np.float32),
            "dyadic-grid": (np.round(cont * 8.0) / 8.0).astype(np.float32)}, (centre / 1.5).astype(np.int64), rng


@pytest.mark.parametrize("kn", [1, 3, 7])
def test_restatement_equals_compute_mi_cd_bit_for_bit(kn):
    mi_mod = pytest.importorskip("sklearn.feature_selection._mutual_info")
    S = 700
    psi = _scipy_psi(S)
    columns, follows, rng = _columns(S, 5)
    labels = {"three-classes": follows, "forty-classes": rng.integers(0, 40, S), "independent": rng.integers(0, 5, S)}
    seen_positive = seen_zero = 0
    for cname, x in columns.items():
        for lname, v in labels.items():
            ours = R.estimate(x, v, kn, psi)
            theirs = mi_mod._compute_mi_cd(x.astype(np.float64), v, kn)
            assert np.float64(ours["mi"]).tobytes() == np.float64(theirs).tobytes(), (cname, lname, ours["mi"], theirs)
            brute = R.estimate(x, v, kn, psi, brute=True)                # the two statements of the integers agree
            assert np.array_equal(brute["m_i"], ours["m_i"]) and np.array_equal(brute["k_i"], ours["k_i"]) and brute["n"] == ours["n"] == S
            seen_positive += ours["mi"] > 0
            seen_zero += ours["mi"] == 0
            if cname == "constant":
                assert (ours["m_i"] == S).all() and ours["mi"] == 0.0     # every row at distance 0: m_i = n, the estimate clips
    assert seen_positive >= 3 and seen_zero >= 3


def test_restatement_equals_compute_mi_cd_with_singletons_and_small_classes():
    mi_mod = pytest.importorskip("sklearn.feature_selection._mutual_info")
    rng = np.random.default_rng(9)
    S = 300
    psi = _scipy_psi(S)
    x = np.round(rng.standard_normal(S) * 16.0).astype(np.float32) / np.float32(16.0)
    # classes of 1 row (dropped), of 2 and of 3 rows (k_i = 1 and 2 below n_neighbors = 3) and large ones
    v = np.concatenate([np.arange(10), np.repeat(np.arange(10, 20), 2), np.repeat(np.arange(20, 30), 3), rng.integers(30, 33, S - 60)])
    v = v[rng.permutation(S)]
    ours = R.estimate(x, v, 3, psi)
    assert ours["n"] == S - 10 and sorted(set(ours["k_i"].tolist())) == [0, 1, 2, 3] and (ours["m_i"][ours["k_i"] == 0] == 0).all()
    assert np.float64(ours["mi"]).tobytes() == np.float64(mi_mod._compute_mi_cd(x.astype(np.float64), v, 3)).tobytes()
    brute = R.estimate(x, v, 3, psi, brute=True)
    assert np.array_equal(brute["m_i"], ours["m_i"]) and np.array_equal(brute["k_i"], ours["k_i"])
    # every label a singleton: nothing is kept and the estimate is 0 (scikit-learn's mean of nothing is not a number: ours is the rule)
    alone = R.estimate(x, np.arange(S), 3, psi)
    assert alone["n"] == 0 and alone["mi"] == 0.0 and alone["raw"] == 0.0 and not alone["m_i"].any()
    # the strict `<`: rows at 0, 1, 2 of one class, kn = 1: r = 1 for each, and only the row itself is strictly nearer
    e = R.estimate(np.array([0.0, 1.0, 2.0], dtype=np.float32), np.zeros(3, dtype=np.int64), 1, psi)
    assert e["m_i"].tolist() == [1, 1, 1]
    # -0 equals +0 and a repeated value is at distance 0 (rows 0, 1: r = 0, the three zeros); rows 2 .. 4: r = 5, strictly
    e = R.estimate(np.array([0.0, -0.0, 0.0, 5.0, 5.0], dtype=np.float32), np.array([0, 0, 1, 1, 0]), 1, psi)
    assert e["m_i"].tolist() == [3, 3, 3, 2, 2] and e["k_i"].tolist() == [1, 1, 1, 1, 1]


def test_digamma_integers_against_scipy():
    n = _knnlib.MAX_ROWS
    want = _scipy_psi(n)
    got = E.digamma_integers(n)
    assert got.dtype == np.float64 and got.shape == (n + 1,) and got[0] == 0.0
    ulps = np.abs(got[1:] - want[1:]) / np.spacing(np.abs(want[1:]))
    print("digamma_integers(%d): at most %.2f ulp from scipy.special.digamma" % (n, ulps.max()))
    assert ulps.max() <= 2.0
    assert got[1] == -0.5772156649015329 and np.array_equal(E.digamma_integers(5), got[:6])
    assert not re.search(r"^\s*(?:import|from)\s+scipy", open(E.__file__).read(), re.M)     # production code does not import it
    with pytest.raises(ValueError, match="at least 1"):
        E.digamma_integers(0)


# ---- 2. the scores ---------------------------------------------------------------------------------------------------------------------
def _scores_agree(raw, H):
    got, want = E.knn_information_scores_from_mi(raw, H), R.scores(raw, H)
    for key in ("mig", "mig_sup", "dcimig", "modularity", "infom", "infoc"):
        assert got[key] == pytest.approx(want[key], abs=1e-14), key
    assert got["n_active"] == want["n_active"] and np.array_equal(got["best_latent"], want["best_latent"])
    return got


def test_scores_of_ideal_rotated_and_degenerate_matrices():
    H = np.array([np.log(3.0), np.log(5.0), np.log(4.0)])
    ideal = np.zeros((5, 3))
    ideal[0, 0], ideal[1, 1], ideal[2, 2] = 0.98 * H                       # latent k holds factor k, two latents hold nothing
    got = _scores_agree(ideal, H)
    assert got["infom"] == 1.0 and got["infoc"] == 1.0 and got["modularity"] == pytest.approx(3 / 5) and got["n_active"] == 3
    assert got["mig"] == pytest.approx(0.98) and got["mig_sup"] == pytest.approx(0.98 * 3 / 5) and got["best_latent"].tolist() == [0, 1, 2]
    assert got["dcimig"] == pytest.approx(0.98)
    rotated = ideal.copy()                                                  # latents 0 and 1 each hold half of factors 0 and 1
    rotated[0, :2] = rotated[1, :2] = 0.5 * H[:2]
    low = _scores_agree(rotated, H)
    assert low["infom"] < 0.7 and low["infoc"] < 0.85 and low["mig"] < 0.4 and low["modularity"] < got["modularity"]
    # clipping happens here, and raw is returned as it came
    neg = ideal.copy()
    neg[3] = -0.01
    clipped = _scores_agree(neg, H)
    assert clipped["n_active"] == 3 and (clipped["mutual_information"][3] == 0).all() and (clipped["raw"][3] == -0.01).all()
    assert clipped["infom"] == 1.0 and clipped["mig"] == got["mig"]
    # K = 1: the InfoM entry's denominator is 0 -> 1.0; one active latent: the InfoC entries are 1.0
    one = _scores_agree(np.array([[0.3], [0.1], [0.0]]), [np.log(2.0)])
    assert one["infom"] == 1.0 and one["n_active"] == 2 and one["infoc"] == pytest.approx((0.75 - 0.5) / 0.5) and one["modularity"] == pytest.approx(2 / 3)
    single = _scores_agree(np.array([[0.0, 0.0], [0.2, 0.1]]), [1.0, 1.0])
    assert single["n_active"] == 1 and single["infoc"] == 1.0 and single["infom"] == pytest.approx((2 / 3 - 0.5) / 0.5)
    # no active latent: both are 0.0; a factor no latent knows is left out of InfoC
    none = _scores_agree(np.zeros((4, 2)), [1.0, 2.0])
    assert none["infom"] == none["infoc"] == none["mig"] == none["modularity"] == 0.0 and none["n_active"] == 0
    part = _scores_agree(np.array([[0.4, 0.0], [0.1, 0.0]]), [1.0, 1.0])
    assert part["infoc"] == pytest.approx((0.8 - 0.5) / 0.5) and part["infom"] == 1.0
    for bad_mi, bad_H, msg in ((np.zeros(3), [1.0], "non-empty"), (np.zeros((2, 2)), [1.0], "non-empty"), (np.zeros((0, 2)), [1.0, 1.0], "non-empty"),
                               (np.full((2, 2), np.nan), [1.0, 1.0], "finite"), (np.zeros((2, 2)), [1.0, 0.0], r"factor\(s\) \[1\] take one value")):
        with pytest.raises(ValueError, match=msg):
            E.knn_information_scores_from_mi(bad_mi, bad_H)


def test_scores_of_an_ideal_and_a_rotated_table_on_the_restatement():
    sizes = (3, 4, 5)
    rng = np.random.default_rng(2)
    vals = R.factor_values(np.arange(60), sizes).astype(np.float64)
    ideal = (vals.T + 0.05 * rng.standard_normal((60, 3))).astype(np.float32)       # latent k is factor k and a little noise
    c = np.sqrt(0.5)
    rotated = ideal.copy()
    rotated[:, 0], rotated[:, 1] = c * (ideal[:, 0] - ideal[:, 1]), c * (ideal[:, 0] + ideal[:, 1])     # 45 degrees
    psi = E.digamma_integers(60)
    got = {}
    for name, tab in (("ideal", ideal), ("rotated", rotated)):
        ref = R.reference(tab, sizes, np.arange(60), 3, psi)
        H = [R.factor_entropy(cnt) for cnt in ref["counts"]]
        got[name] = E.knn_information_scores_from_mi(ref["raw"], H)
        assert np.array_equal(got[name]["raw"], R.raw_from_sums(ref["n"], ref["sums"], psi))
    print({k: {s: round(v[s], 3) for s in ("mig", "infom", "infoc", "modularity")} for k, v in got.items()})
    assert got["ideal"]["best_latent"].tolist() == [0, 1, 2] and got["ideal"]["mig"] >= 0.6
    assert got["ideal"]["infom"] >= 0.8 and got["ideal"]["infoc"] >= 0.8
    for key in ("mig", "infom", "infoc"):
        assert got["rotated"][key] < got["ideal"][key] - 0.05, key


# ---- 3. the library ------------------------------------------------------------------------------------------------------------------
def test_header_ctypes_table_and_exports_agree(monkeypatch):
    declared = sorted(set(re.findall(r"\b(dvae_knn_[a-zA-Z0-9_]+)\s*\(", _header())))
    assert declared == sorted(_knnlib.SIGNATURES)
    assert declared == sorted(["dvae_knn_version", "dvae_knn_last_error", "dvae_knn_ws_bytes", "dvae_knn_sort", "dvae_knn_mi"])
    exported = sorted(set(re.findall(r" T (dvae_\w+)", _nm(os.path.abspath(_knnlib.LIB_PATH), "-D", "--defined-only"))))
    assert exported == declared
    assert re.findall(r" U (dvae_\w+)", _nm(os.path.abspath(_knnlib.LIB_PATH), "-D")) == []
    kinds = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_long: "l", ctypes.c_double: "d"}
    for name, params in re.findall(r"\b(dvae_knn_[a-zA-Z0-9_]+)\s*\(([^)]*)\)", _header()):
        got = []
        for prm in [x.strip() for x in params.split(",") if x.strip() != "void"]:
            got.append("p" if "*" in prm else ("l" if prm.startswith("long") else "d" if prm.startswith("double") else "i"))
        assert got == [kinds[t] for t in _knnlib.SIGNATURES[name]], name
    macros = {k: int(v) for k, v in re.findall(r"#define (DVAE_KNN_\w+) (\d+)", _header())}
    mirrored = {"DVAE_KNN_VERSION": _knnlib.VERSION, "DVAE_KNN_MAX_FACTORS": _knnlib.MAX_FACTORS, "DVAE_KNN_MAX_CLASSES": _knnlib.MAX_CLASSES,
                "DVAE_KNN_MAX_NEIGHBORS": _knnlib.MAX_NEIGHBORS, "DVAE_KNN_MAX_D": _knnlib.MAX_D, "DVAE_KNN_MAX_ROWS": _knnlib.MAX_ROWS,
                "DVAE_KNN_SORT_THREADS": _knnlib.SORT_THREADS, "DVAE_KNN_SORT_ROW_BYTES": _knnlib.SORT_ROW_BYTES,
                "DVAE_KNN_MI_THREADS": _knnlib.MI_THREADS, "DVAE_KNN_MI_ROW_BYTES": _knnlib.MI_ROW_BYTES,
                "DVAE_KNN_MI_FIXED_BYTES": _knnlib.MI_FIXED_BYTES}
    assert macros == mirrored                                            # every macro of the header, none besides
    # the limits of the issue: DCI's 10 240 rows, 256 values, eight factors, 64 neighbours, D as the SAP library's
    assert _knnlib.MAX_ROWS >= 10240 and _knnlib.MAX_CLASSES == 256 and _knnlib.MAX_FACTORS == _infolib.MAX_FACTORS == 8
    assert _knnlib.MAX_NEIGHBORS == 64 and _knnlib.MAX_D == _saplib.MAX_D
    # the LDS plan of both kernels at the row limit fits the 160 KiB of a compute unit
    sort_bytes, mi_bytes = _knnlib.lds_bytes(_knnlib.MAX_ROWS)
    assert sort_bytes == 8 * _knnlib.MAX_ROWS <= 160 * 1024 and mi_bytes == 9 * _knnlib.MAX_ROWS + _knnlib.MI_FIXED_BYTES <= 160 * 1024
    assert _knnlib.lds_bytes(10000) == (8 * 16384, 90000 + _knnlib.MI_FIXED_BYTES) and _knnlib.lds_bytes(1) == (8, 9 + _knnlib.MI_FIXED_BYTES)
    assert _knnlib.MAX_ROWS <= 65536                                       # places and selection indices are uint16 in LDS
    h = _knnlib.lib()
    assert h.dvae_knn_version() == _knnlib.VERSION == 1
    assert h.dvae_knn_ws_bytes(60, 3, 0) == 8 * 3 * 60 and h.dvae_knn_ws_bytes(737280, 10, 10000) == 800000
    assert h.dvae_knn_ws_bytes(737280, 10, 0) == 0 and h.dvae_knn_ws_bytes(60, 0, 10) == 0 and h.dvae_knn_ws_bytes(60, 3, _knnlib.MAX_ROWS + 1) == 0
    binding = open(_knnlib.__file__).read()
    assert 'Binding.for_library("knn", SIGNATURES, _RESTYPE' in binding and "LIB_PATH = _binding.path" in binding
    assert _knnlib._binding.last_error == "dvae_knn_last_error" and _knnlib._binding.signatures is _knnlib.SIGNATURES
    assert _knnlib._binding.soname == "libdvae_knn_hip.so"
    monkeypatch.setenv("DVAE_KNN_HIP_LIB", "/elsewhere/lib.so")            # the override, read when a binding is made
    assert _cabi.Binding.for_library("knn", {}, {}, "", subdir=os.path.join("..", "lib_scores")).path == "/elsewhere/lib.so"
    monkeypatch.delenv("DVAE_KNN_HIP_LIB")
    assert os.path.normpath(_knnlib.LIB_PATH).endswith(os.path.join("disentangling-vae_amd", "lib_scores", "libdvae_knn_hip.so"))
    for name in ("knn_information_scores_from_table", "knn_information_scores_from_mi", "digamma_integers"):
        assert name in disvae_amd.__all__ and getattr(disvae_amd, name) is getattr(E, name)


def test_build_has_the_row_in_its_list_and_the_library_in_its_directory():
    """IN the list and IN the directory: nothing here says that either holds one entry, so the next score library is one more row."""
    build = _build()
    assert ("knn", ["knn_mi"], "dvae_knn_hip.h") in [tuple(row) for row in build.SCORE_TARGETS]
    assert "one more row of THIS list" in open(os.path.join(ROOT, "disentangling-vae_amd", "build.py")).read()
    for other in (build.TARGETS, build.PLUGIN_TARGETS, build.SCORE_PLUGIN_TARGETS, build.EXTRA_TARGETS, build.MORE_TARGETS):
        assert "knn" not in [row[0] for row in other]
    assert "knn_mi" not in build.ALL_SOURCES and "knn_mi" not in open(os.path.join(ROOT, "tools", "isa_identity.py")).read()
    assert build.KNN_SOURCES == ["knn_mi"] and os.path.exists(os.path.join(build.SRC, SOURCE))
    pkg = os.path.join(ROOT, "disentangling-vae_amd")
    assert os.path.abspath(build.KNN_LIB) == os.path.join(pkg, "lib_scores", "libdvae_knn_hip.so") and os.path.exists(build.KNN_LIB)
    assert os.path.abspath(build.KNN_LIB) == os.path.abspath(_knnlib.LIB_PATH)
    assert "libdvae_knn_hip.so" in os.listdir(os.path.join(pkg, "lib_scores"))
    assert sorted(os.path.basename(h) for h in build.KNN_HEADERS if "include" in h.split(os.sep)) == ["dvae_hip.h", "dvae_knn_hip.h"]
    row = [r for r in build.SCORE_TARGETS if r[0] == "knn"][0]
    assert build._target(*row, subdir=build.SCORE_DIR)[3] == os.path.join(build.OBJ, "flags_knn.txt")
    assert open(os.path.join(build.OBJ, "flags_knn.txt")).read() == open(os.path.join(build.OBJ, "flags_sap.txt")).read().replace(
        "svm_1d", "knn_mi")                                               # build() stamped it: the same flags and stamp logic
    ignored = subprocess.run(["git", "check-ignore", "-q", build.KNN_LIB], cwd=ROOT).returncode
    assert ignored in (0, 128)                                            # ignored like lib/ (128: not a git checkout)
    src = open(os.path.join(CSRC, SOURCE)).read()
    assert sorted(re.findall(r'^#include "([^"]+)"', src, re.M)) == ["../../include/dvae_knn_hip.h", "common.h", "last_error.h"]


def test_source_obeys_the_rules_of_the_score_libraries():
    src = open(os.path.join(CSRC, SOURCE)).read()
    assert len(re.findall(r'^#include "last_error\.h"', src, re.M)) == 1
    assert not re.search(r"\bthread_local\b", src) and not re.search(r"^void set_error\(", src, re.M)
    for name in ("put_f64", "get_f64", "chunks_of", "lesser"):              # table_stats.h is their one home
        assert not re.search(r"^[ \w]*\b(?:void|double|int|T)\s+%s\s*\([^;{]*\)\s*\{" % name, src, re.M), name
    code = re.sub(r"//[^\n]*", "", src.split("#include", 1)[1])
    atomics = re.findall(r"atomic\w*\s*\(([^;]*);", code)
    assert atomics == ["&f.cnt[v], 1)"]                                     # the one atomic: an integer add on the LDS class counts
    assert re.search(r"\bint cnt\[KNN_C\];", code)
    assert "while" not in code and "hipLaunchCooperativeKernel" not in src  # bounded loops only, no cooperative launch
    assert not re.search(r"hipMalloc|hipFree|hipMemcpy|hipMemset|Synchronize", src)    # the entry points only enqueue
    for bound in ("it < KNN_BISECT", "s < kk", "k <= P2", "base < S"):
        assert bound in code
    assert "labels" not in re.findall(r"k_knn_mi\(([^)]*)\)", code)[0]      # labels never exist in global memory


def _put(good, i, v):
    return good[:i] + [v] + good[i + 1:]


def test_bad_arguments_are_refused_before_a_launch_with_the_librarys_own_text():
    h = _knnlib.lib()
    assert h is _knnlib.lib()                                              # loaded once
    sizes = _knnlib.host_sizes([3, 2])
    #       table  rows   N  D  S  ws     stream
    sort = [DUMMY, DUMMY, 6, 3, 4, DUMMY, None]
    #     rows   sizes  N  D  K  S  kn psi    ws     sums   counts m_of  k_of  stream
    mi = [DUMMY, sizes, 6, 3, 2, 4, 3, DUMMY, DUMMY, DUMMY, DUMMY, None, None, None]
    bad_sort = [_put(sort, 0, None), _put(sort, 5, None), _put(sort, 2, 0), _put(sort, 2, 2 ** 31), _put(sort, 3, 0),
                _put(sort, 3, _knnlib.MAX_D + 1), _put(sort, 4, 0), _put(sort, 4, _knnlib.MAX_ROWS + 1),
                _put(_put(sort, 1, None), 2, _knnlib.MAX_ROWS + 1)]        # rows = NULL: S = N, above the limit
    bad_mi = [_put(mi, i, None) for i in (1, 7, 8, 9, 10)]
    bad_mi += [_put(mi, 2, 0), _put(mi, 2, 7), _put(mi, 3, 0), _put(mi, 3, _knnlib.MAX_D + 1), _put(mi, 4, 0), _put(mi, 4, 9), _put(mi, 5, 0),
               _put(mi, 5, _knnlib.MAX_ROWS + 1), _put(mi, 6, 0), _put(mi, 6, _knnlib.MAX_NEIGHBORS + 1),
               _put(mi, 1, _knnlib.host_sizes([3, 0])), _put(mi, 1, _knnlib.host_sizes([257, 2])), _put(mi, 1, _knnlib.host_sizes([3, 3])),
               _put(_put(mi, 1, _knnlib.host_sizes([256] * 8)), 4, 8)]   # a product beyond 2^63 is not N either
    for name, cases in (("dvae_knn_sort", bad_sort), ("dvae_knn_mi", bad_mi)):
        for args in cases:
            with pytest.raises(_lib.DvaeHipError) as e:
                _knnlib.call(name, *args)
            own = h.dvae_knn_last_error().decode()
            assert "invalid argument" in own and SOURCE in own, (args, own)
            assert str(e.value) == "%s failed (-1): %s" % (name, own)
    with pytest.raises(_lib.DvaeHipError, match=r"S >= 1 && S <= DVAE_KNN_MAX_ROWS"):      # the row limit, in the library's own words
        _knnlib.call("dvae_knn_sort", *_put(sort, 4, _knnlib.MAX_ROWS + 1))
    with pytest.raises(_lib.DvaeHipError, match=r"rows_enumerated == N"):
        _knnlib.call("dvae_knn_mi", *_put(mi, 2, 7))
    assert SOURCE not in _infolib.lib().dvae_info_last_error().decode()    # every library keeps its own buffer


def test_call_loads_through_the_modules_lib(monkeypatch):
    class Boom(Exception):
        pass

    def boom():
        raise Boom("lib() of the module was asked")
    monkeypatch.setattr(_knnlib, "lib", boom)
    with pytest.raises(Boom, match="was asked"):
        _knnlib.call("dvae_knn_version")


# ---- 4. errors before any library call -------------------------------------------------------------------------------------------
class _Factors:
    lat_sizes = np.array([3, 2])
    lat_names = ("a", "b")

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


class _Loader:
    def __init__(self, dataset, batches):
        self.dataset, self.batches = dataset, batches

    def __iter__(self):
        if self.batches is None:
            raise AssertionError("iterated before the sizes were checked")
        return iter(self.batches)


class _Model(torch.nn.Module):
    latent_dim = 2

    def __init__(self):
        super().__init__()
        self.modes = []

    def encoder(self, x):
        self.modes.append(self.training)
        return torch.zeros(x.shape[0], 2), torch.zeros(x.shape[0], 2)


def test_argument_errors_raise_before_any_library_call(monkeypatch):
    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_knnlib, "lib", no_library)
    mean = torch.zeros(6, 4)
    ok = dict(n_samples=5)
    for sizes, kw, msg in (([3, 3], ok, "does not enumerate"), ([3, 2], dict(n_samples=0), r"n_samples must lie in \[1, %d\]" % _knnlib.MAX_ROWS),
                           ([3, 2], dict(n_samples=_knnlib.MAX_ROWS + 1), r"n_samples must lie in \[1, %d\]" % _knnlib.MAX_ROWS),
                           ([3, 2], {}, "n_samples must be at most 6"), ([3, 2], dict(n_samples=7), "n_samples must be at most 6"),
                           ([2] * 9, ok, "at most 8"), ([0, 2], ok, "positive sizes"), ([6, 1], ok, "one value has no entropy"),
                           ([3, 2], dict(ok, n_neighbors=0), r"n_neighbors must be an integer in \[1, 64\]"),
                           ([3, 2], dict(ok, n_neighbors=65), "n_neighbors must be"), ([3, 2], dict(ok, n_neighbors=2.5), "n_neighbors must be"),
                           ([3, 2], dict(rows=[0, 1, 2, 6]), r"in \[0, 6\)"), ([3, 2], dict(rows=[]), "rows must hold between 1 and"),
                           ([3, 2], dict(rows=np.zeros(_knnlib.MAX_ROWS + 1, dtype=np.int64)), "rows must hold between 1 and %d" % _knnlib.MAX_ROWS)):
        with pytest.raises(ValueError, match=msg):
            E.knn_information_scores_from_table(mean, sizes, **kw)
    with pytest.raises(ValueError, match="at most %d" % _knnlib.MAX_CLASSES):
        E.knn_information_scores_from_table(torch.zeros(514, 1), [257, 2], n_samples=10)
    with pytest.raises(ValueError, match="table"):
        E.knn_information_scores_from_table(torch.zeros(6), [3, 2], **ok)
    with pytest.raises((TypeError, ValueError)):
        E.knn_information_scores_from_table(mean, [3, 2], seed="x", **ok)
    bad = mean.clone()
    bad[4, 1] = float("nan")
    with pytest.raises(ValueError, match="NaN or an infinity"):
        E.knn_information_scores_from_table(bad, [3, 2], **ok)
    with pytest.raises(_lib.DvaeHipError, match="no CPU"):
        E.knn_information_scores_from_table(mean, [3, 2], **ok)
    with pytest.raises(_lib.DvaeHipError, match="no CPU"):                 # repeats in rows are allowed
        E.knn_information_scores_from_table(mean, [3, 2], rows=[0, 0, 5, 5, 1])
    model = _Model().train()
    ev = E.Evaluator(model, None, is_progress_bar=False)
    with pytest.raises(ValueError, match="known true factors"):
        ev.compute_knn_information_scores(_Loader([0, 1, 2], None))
    for kw, msg in ((dict(n_samples=0), "n_samples must lie"), ({}, "n_samples must be at most 6"), (dict(ok, n_neighbors=0), "n_neighbors must be")):
        with pytest.raises(ValueError, match=msg):
            ev.compute_knn_information_scores(_Loader(_Factors(6), None), **kw)
    with pytest.raises(ValueError, match=r"data set of 5 images does not enumerate lat_sizes=\[3, 2\]"):
        ev.compute_knn_information_scores(_Loader(_Factors(5), None), **ok)
    assert model.modes == [] and model.training
    loader = _Loader(_Factors(6), [(torch.rand(4, 1), None), (torch.rand(2, 1), None)])
    with pytest.raises(_lib.DvaeHipError, match="no CPU"):                 # valid arguments: the table is on the CPU
        ev.compute_knn_information_scores(loader, **ok)
    assert model.modes == [False, False] and model.training               # encoded in eval mode, and the mode is as it was


def test_call_writes_the_knn_information_scores_on_request(monkeypatch, tmp_path):
    seen = []
    model = _Model().train()
    ev = E.Evaluator(model, None, is_progress_bar=False, save_dir=str(tmp_path))
    result = {"mig": 0.5, "infom": 0.75, "infoc": 0.25, "n_active": 2, "best_latent": np.array([0, 1]), "mutual_information": np.ones((2, 2)),
              "raw": np.ones((2, 2)), "n_kept": np.full((2, 2), 6), "factor_entropy": np.array([1.0, 0.5]), "n_samples": 6, "n_neighbors": 3}
    monkeypatch.setattr(ev, "compute_knn_information_scores", lambda loader, **kw: seen.append((loader, kw, model.training)) or result)
    monkeypatch.setattr(ev, "compute_losses", lambda loader: {"loss": 1.5})
    loader = object()
    assert ev(loader) == (None, {"loss": 1.5}) and seen == [] and os.listdir(tmp_path) == ["test_losses.log"]
    assert ev(loader, is_losses=False, is_knn_information=True) == (None, None)
    assert seen == [(loader, {}, False)] and model.training
    assert ev(loader, is_losses=False, is_knn_information=True, knn_information_args=dict(n_samples=6, n_neighbors=1)) == (None, None)
    assert seen[-1] == (loader, dict(n_samples=6, n_neighbors=1), False)
    assert E.KNN_INFORMATION_SCORES_FILE == "knn_information_scores.log"
    assert json.load(open(tmp_path / "knn_information_scores.log")) == {
        "mig": 0.5, "infom": 0.75, "infoc": 0.25, "n_active": 2, "best_latent": [0, 1], "factor_entropy": [1.0, 0.5], "n_samples": 6,
        "n_neighbors": 3}                                                 # without the [D, K] matrices
