"""CPU: the host side of the linear-softmax probes -- the fifteenth library's C-ABI (include/dvae_lr_hip.h == disvae_amd/_lrlib.py ==
the built lib_scores/libdvae_lr_hip.so), its row of build.py's SCORE_TARGETS (asserted to be IN the list and IN the directory, never
to be all of either), the rules its source obeys, the refusal of bad arguments before any launch, the restatement tests/lr_ref.py
against fit_logistic_regression and the installed scikit-learn, the head-room of every test table under the solver's iteration
bound, InfoE from cross-entropies, and the argument errors of the public functions before any device work.

Measured here (scikit-learn 1.7.2, the tables of AGREEMENT below, C = 1):
    coefficients of the reference optimum (b centred) against fit_logistic_regression: at most 5.4e-7 apart; against
    LogisticRegression(C=1.0, tol=1e-10, max_iter=10000): at most 9.0e-7 -- both inside the 3.3e-5 that DESIGN.md records for two
    converged optimisers; the objective at the reference optimum is never above either's.
    Newton steps of the reference solve: at most 11; of the device's iteration restated (lr_ref.newton_cg): at most 16 of 100.
"""
import ctypes
import importlib.util
import json
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest
import torch

import lr_ref as R
import sap_ref as SR
import disvae_amd
from disvae_amd import _cabi, _infolib, _knnlib, _lib, _lrlib
from disvae_amd import evaluate as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dvae_lr_hip.h")
CSRC = os.path.join(ROOT, "disentangling-vae_amd", "csrc")
SOURCE = "softmax_fit.hip"
DUMMY = 1 << 20                                                   # aligned non-NULL address, never dereferenced
SPREAD = 3.3e-5                                                   # two converged optimisers
AGREEMENT = ["rows-63", "rows-65-five-problems", "rows-511-duplicates", "rows-513-one-row-class", "d17", "separable-257", "offset-scaled",
             "constant-zero-column"]


def _build():
    spec = importlib.util.spec_from_file_location("dvae_build_lr", os.path.join(ROOT, "disentangling-vae_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _nm(path, *flags):
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin")
    assert nm, "no nm on this machine"
    return subprocess.run([nm] + list(flags) + [path], capture_output=True, text=True, check=True).stdout


# ---- 1. the library -----------------------------------------------------------------------------------------------------------
def test_header_ctypes_table_and_exports_agree(monkeypatch):
    declared = sorted(set(re.findall(r"\b(dvae_lr_[a-zA-Z0-9_]+)\s*\(", _header())))
    assert declared == sorted(_lrlib.SIGNATURES)
    assert declared == sorted(["dvae_lr_version", "dvae_lr_last_error", "dvae_lr_ws_bytes", "dvae_lr_fit", "dvae_lr_predict"])
    exported = sorted(set(re.findall(r" T (dvae_\w+)", _nm(os.path.abspath(_lrlib.LIB_PATH), "-D", "--defined-only"))))
    assert exported == declared
    assert re.findall(r" U (dvae_\w+)", _nm(os.path.abspath(_lrlib.LIB_PATH), "-D")) == []
    kinds = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_long: "l", ctypes.c_double: "d"}
    for name, params in re.findall(r"\b(dvae_lr_[a-zA-Z0-9_]+)\s*\(([^)]*)\)", _header()):
        got = []
        for prm in [x.strip() for x in params.split(",") if x.strip() != "void"]:
            got.append("p" if "*" in prm else ("l" if prm.startswith("long") else "d" if prm.startswith("double") else "i"))
        assert got == [kinds[t] for t in _lrlib.SIGNATURES[name]], name
    assert _lrlib._RESTYPE["dvae_lr_ws_bytes"] is ctypes.c_long and re.search(r"\blong dvae_lr_ws_bytes\(", _header())
    macros = {k: int(v) for k, v in re.findall(r"#define (DVAE_LR_\w+) (\d+)", _header())}
    mirrored = {"DVAE_LR_VERSION": _lrlib.VERSION, "DVAE_LR_MAX_ROWS": _lrlib.MAX_ROWS, "DVAE_LR_MAX_D": _lrlib.MAX_D,
                "DVAE_LR_MAX_CLASSES": _lrlib.MAX_CLASSES, "DVAE_LR_MAX_PROBLEMS": _lrlib.MAX_PROBLEMS, "DVAE_LR_THREADS": _lrlib.THREADS,
                "DVAE_LR_FEATURE_TILE": _lrlib.FEATURE_TILE, "DVAE_LR_CHUNK_ROWS": _lrlib.CHUNK_ROWS,
                "DVAE_LR_PREDICT_THREADS": _lrlib.PREDICT_THREADS, "DVAE_LR_MAX_ITERATIONS": _lrlib.MAX_ITERATIONS,
                "DVAE_LR_MAX_CG": _lrlib.MAX_CG, "DVAE_LR_MAX_HALVINGS": _lrlib.MAX_HALVINGS}
    assert macros == mirrored                                            # every macro of the header, none besides
    assert (R.THREADS, R.CHUNK_ROWS, R.PREDICT_THREADS) == (_lrlib.THREADS, _lrlib.CHUNK_ROWS, _lrlib.PREDICT_THREADS)
    assert (R.MAX_ITERATIONS, R.MAX_CG, R.MAX_HALVINGS) == (_lrlib.MAX_ITERATIONS, _lrlib.MAX_CG, _lrlib.MAX_HALVINGS)
    # the issue's limits
    assert (_lrlib.MAX_ROWS, _lrlib.MAX_D, _lrlib.MAX_CLASSES, _lrlib.MAX_PROBLEMS) == (16384, 64, 256, 8)
    assert "sum_c b_c = 0" in open(HEADER).read()                        # the header says where the solver stays
    assert _lrlib.lib().dvae_lr_version() == _lrlib.VERSION == 1
    binding = open(_lrlib.__file__).read()
    assert 'Binding.for_library("lr", SIGNATURES, _RESTYPE' in binding and "LIB_PATH = _binding.path" in binding
    assert _lrlib._binding.last_error == "dvae_lr_last_error" and _lrlib._binding.signatures is _lrlib.SIGNATURES
    assert _lrlib._binding.soname == "libdvae_lr_hip.so"
    monkeypatch.setenv("DVAE_LR_HIP_LIB", "/elsewhere/lib.so")             # the override, read when a binding is made
    assert _cabi.Binding.for_library("lr", {}, {}, "", subdir=os.path.join("..", "lib_scores")).path == "/elsewhere/lib.so"
    monkeypatch.delenv("DVAE_LR_HIP_LIB")
    assert os.path.normpath(_lrlib.LIB_PATH).endswith(os.path.join("disentangling-vae_amd", "lib_scores", "libdvae_lr_hip.so"))
    assert os.path.normpath(_knnlib.LIB_PATH).endswith(os.path.join("lib_scores", "libdvae_knn_hip.so"))        # as before
    for name in ("fit_logistic_regression_device", "infoe_from_table", "infoe_from_log_loss"):
        assert name in disvae_amd.__all__ and getattr(disvae_amd, name) is getattr(E, name)
    for S, C, D in ((2, 2, 1), (63, 3, 3), (65, 5, 10), (512, 256, 2), (16384, 2, 2), (10000, 40, 10), (1025, 2, 1)):
        n_chunks, chunk = _lrlib.chunks(S, C, D)
        assert (n_chunks, chunk) == R.chunks(S, C, D) and (n_chunks - 1) * chunk < S <= n_chunks * chunk     # none of them empty
        want = 8 * (2 * C * S + n_chunks * C * (D + 1) + 8 * C * (D + 1))
        assert _lrlib.lib().dvae_lr_ws_bytes(S, D, _lrlib.host_classes([C]), 1) == want


def test_build_has_the_row_and_the_library_lies_in_lib_scores():
    build = _build()
    assert ("lr", ["softmax_fit"], "dvae_lr_hip.h") in [tuple(row) for row in build.SCORE_TARGETS]
    assert ("knn", ["knn_mi"], "dvae_knn_hip.h") in [tuple(row) for row in build.SCORE_TARGETS]                 # as before
    assert "softmax_fit" not in build.ALL_SOURCES and len(build.ALL_SOURCES) == 31
    assert "softmax_fit" not in open(os.path.join(ROOT, "tools", "isa_identity.py")).read()
    assert build.LR_SOURCES == ["softmax_fit"] and os.path.exists(os.path.join(build.SRC, SOURCE))
    pkg = os.path.join(ROOT, "disentangling-vae_amd")
    assert os.path.abspath(build.LR_LIB) == os.path.join(pkg, "lib_scores", "libdvae_lr_hip.so") and os.path.exists(build.LR_LIB)
    assert os.path.abspath(build.LR_LIB) == os.path.abspath(_lrlib.LIB_PATH)
    assert "libdvae_lr_hip.so" in os.listdir(os.path.join(pkg, "lib_scores"))
    assert sorted(os.path.basename(h) for h in build.LR_HEADERS if "include" in h.split(os.sep)) == ["dvae_hip.h", "dvae_lr_hip.h"]
    row = [r for r in build.SCORE_TARGETS if r[0] == "lr"][0]
    assert build._target(*row, subdir=build.SCORE_DIR)[3] == os.path.join(build.OBJ, "flags_lr.txt")
    assert open(os.path.join(build.OBJ, "flags_lr.txt")).read() == open(os.path.join(build.OBJ, "flags_knn.txt")).read().replace(
        "knn_mi", "softmax_fit")                                          # build() stamped it: the same flags and stamp logic
    ignored = subprocess.run(["git", "check-ignore", "-q", build.LR_LIB], cwd=ROOT).returncode
    assert ignored in (0, 128)                                            # ignored like lib/ (128: not a git checkout)
    src = open(os.path.join(CSRC, SOURCE)).read()
    assert sorted(re.findall(r'^#include "([^"]+)"', src, re.M)) == ["../../include/dvae_lr_hip.h", "common.h", "last_error.h", "table_stats.h"]


def test_source_obeys_the_rules_of_the_score_libraries():
    src = open(os.path.join(CSRC, SOURCE)).read()
    assert len(re.findall(r'^#include "last_error\.h"', src, re.M)) == 1
    assert not re.search(r"\bthread_local\b", src) and not re.search(r"^void set_error\(", src, re.M)
    for name in ("put_f64", "get_f64", "chunks_of", "lesser"):              # table_stats.h is their one home; two of them are used here
        assert not re.search(r"^[ \w]*\b(?:void|double|int|T)\s+%s\s*\([^;{]*\)\s*\{" % name, src, re.M), name
    assert "chunks_of(" in src and "lesser(" in src
    code = re.sub(r"//[^\n]*", "", src.split("#include", 1)[1])
    assert not re.search(r"atomic", code)                                   # no atomics of any kind
    assert "while" not in code and "hipLaunchCooperativeKernel" not in src  # bounded loops only, no cooperative launch
    assert not re.search(r"hipMalloc|hipFree|hipMemcpy|hipMemset|Synchronize", src)    # the entry points only enqueue
    assert not re.search(r"\bfloat\s+\w+\s*=|\bexpf\(|\blogf\(", code.split("k_lr_predict")[0])           # the solver is fp64 throughout
    for bound in ("it <= DVAE_LR_MAX_ITERATIONS", "j < DVAE_LR_MAX_CG", "hv <= DVAE_LR_MAX_HALVINGS"):
        assert bound in code
    assert len(re.findall(r"hipLaunchKernelGGL\(", code)) == 2              # one launch per entry point: a whole solve is one


def _put(good, i, v):
    return good[:i] + [v] + good[i + 1:]


def test_bad_arguments_are_refused_before_a_launch_with_the_librarys_own_text():
    h = _lrlib.lib()
    assert h is _lrlib.lib()                                               # loaded once
    cls = _lrlib.host_classes([3, 2])
    #      feat   shift  scale  labels n_cls S  D  Q  C    tol   ws     coef   report stream
    fit = [DUMMY, DUMMY, DUMMY, DUMMY, cls, 6, 3, 2, 1.0, 1e-8, DUMMY, DUMMY, DUMMY, None]
    #      feat   shift  scale  labels n_cls T  D  Q  coef   prob   loss   correct counted stream
    prd = [DUMMY, DUMMY, DUMMY, DUMMY, cls, 6, 3, 2, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, None]
    bad_fit = [_put(fit, i, None) for i in (0, 1, 2, 3, 4, 10, 11, 12)]     # 1, 2: shift without scale and scale without shift
    bad_fit += [_put(fit, 5, 0), _put(fit, 5, _lrlib.MAX_ROWS + 1), _put(fit, 6, 0), _put(fit, 6, _lrlib.MAX_D + 1), _put(fit, 7, 0),
                _put(fit, 7, _lrlib.MAX_PROBLEMS + 1), _put(fit, 8, 0.0), _put(fit, 8, -1.0), _put(fit, 8, float("inf")), _put(fit, 8, float("nan")),
                _put(fit, 9, -1e-9), _put(fit, 9, float("inf")), _put(fit, 9, float("nan")), _put(fit, 10, DUMMY + 4),
                _put(fit, 4, _lrlib.host_classes([3, 0])), _put(fit, 4, _lrlib.host_classes([_lrlib.MAX_CLASSES + 1, 2]))]
    bad_prd = [_put(prd, i, None) for i in (0, 1, 2, 3, 4, 8, 10, 11, 12)]
    bad_prd += [_put(prd, 5, 0), _put(prd, 5, 2 ** 31), _put(prd, 6, 0), _put(prd, 6, 65), _put(prd, 7, 0), _put(prd, 7, 9),
                _put(prd, 4, _lrlib.host_classes([3, -1]))]
    for name, cases in (("dvae_lr_fit", bad_fit), ("dvae_lr_predict", bad_prd)):
        for args in cases:
            with pytest.raises(_lib.DvaeHipError) as e:
                _lrlib.call(name, *args)
            own = h.dvae_lr_last_error().decode()
            assert "invalid argument" in own and SOURCE in own, (args, own)
            assert str(e.value) == "%s failed (-1): %s" % (name, own)
    with pytest.raises(_lib.DvaeHipError, match=r"S >= 1 && S <= DVAE_LR_MAX_ROWS"):        # the row limit, in the library's own words
        _lrlib.call("dvae_lr_fit", *_put(fit, 5, _lrlib.MAX_ROWS + 1))
    assert SOURCE not in _infolib.lib().dvae_info_last_error().decode()    # every library keeps its own buffer
    for S, D, classes in ((0, 3, [2]), (_lrlib.MAX_ROWS + 1, 3, [2]), (5, 0, [2]), (5, 65, [2]), (5, 3, [0]), (5, 3, [257]), (5, 3, [2] * 9)):
        assert h.dvae_lr_ws_bytes(S, D, _lrlib.host_classes(classes), len(classes)) == -1
    assert h.dvae_lr_ws_bytes(5, 3, None, 1) == -1 and h.dvae_lr_ws_bytes(5, 3, _lrlib.host_classes([2]), 0) == -1


def test_call_loads_through_the_modules_lib(monkeypatch):
    class Boom(Exception):
        pass

    def boom():
        raise Boom("lib() of the module was asked")
    monkeypatch.setattr(_lrlib, "lib", boom)
    with pytest.raises(Boom, match="was asked"):
        _lrlib.call("dvae_lr_version")


# ---- 2. the restatement -------------------------------------------------------------------------------------------------------------
def test_gradient_and_hessian_of_the_restatement_by_differences():
    c = R.case("rows-63")
    X, y, C, D = c["X"][:63], c["labels"][1, :63], 3, 3
    rng = np.random.default_rng(0)
    theta = 0.3 * rng.standard_normal(C * (D + 1))
    g, H = R.gradient(X, y, C, 1.0, theta), R.hessian(X, y, C, 1.0, theta)
    for o in range(len(theta)):
        e = np.zeros_like(theta)
        e[o] = 1e-6
        fd = (R.objective(X, y, C, 1.0, theta + e) - R.objective(X, y, C, 1.0, theta - e)) / 2e-6
        assert abs(fd - g[o]) <= 1e-9
        assert np.abs((R.gradient(X, y, C, 1.0, theta + e) - R.gradient(X, y, C, 1.0, theta - e)) / 2e-6 - H[:, o]).max() <= 1e-9
    P, _r = R._residual(X, y, theta, C)
    v = rng.standard_normal(len(theta))
    assert np.abs(R.hessian_vector(X, P, C, 1.0, v) - H @ v).max() <= 1e-14
    assert np.abs(R.hessian_diagonal(X, P, C, 1.0) - np.diag(H)).max() <= 1e-15
    n = R.null_vector(C, D)
    assert np.abs(H @ n).max() <= 1e-16 and abs(g @ n) <= 1e-16            # f does not see a constant added to b
    assert R.objective(X, y, C, 1.0, theta + 5.0 * n) == pytest.approx(R.objective(X, y, C, 1.0, theta), abs=1e-14)


@pytest.mark.parametrize("name", AGREEMENT)
def test_reference_optimum_against_the_host_fit_and_scikit_learn(name):
    linear_model = pytest.importorskip("sklearn.linear_model")
    c = R.case(name)
    S, D = c["S"], c["D"]
    X = c["X"][:S]
    for q, C in enumerate(c["classes"]):
        y, ref = c["labels"][q, :S], c["problems"][q]
        assert ref["gmax"] <= 1e-13 and abs(R.split(ref["theta"], C, D)[1].sum()) <= 1e-12
        f_ref = R.objective(X, y, C, c["reg_C"], ref["theta"])
        W, b = E.fit_logistic_regression(torch.from_numpy(X), torch.from_numpy(y.astype(np.int64)), C, C=c["reg_C"])
        host = R.centred(R.join(W.numpy(), b.numpy()), C, D)
        # Two classes: scikit-learn fits ONE row w (a sigmoid) and penalises ||w||^2, where the two softmax rows (-w / 2, w / 2) of
        # fit_logistic_regression's objective cost ||w||^2 / 2 -- the same model under HALF the penalty, i.e. under 2 C.
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            clf = linear_model.LogisticRegression(C=c["reg_C"] * (2.0 if C == 2 else 1.0), tol=1e-10, max_iter=10000).fit(X, y)
        if C == 2:
            Ws, bs = np.stack([-clf.coef_[0] / 2, clf.coef_[0] / 2]), np.array([-clf.intercept_[0] / 2, clf.intercept_[0] / 2])
        else:
            Ws, bs = clf.coef_, clf.intercept_
        theirs = R.centred(R.join(Ws, bs), C, D)
        d_host, d_sk = float(np.abs(host - ref["theta"]).max()), float(np.abs(theirs - ref["theta"]).max())
        f_host, f_sk = R.objective(X, y, C, c["reg_C"], host), R.objective(X, y, C, c["reg_C"], theirs)
        print("%s[%d]: theta* against the host fit %.2e, against scikit-learn %.2e (allowed %.1e); f* - f_host = %.2e, f* - f_sklearn = %.2e"
              % (name, q, d_host, d_sk, SPREAD, f_ref - f_host, f_ref - f_sk))
        assert d_host <= SPREAD and d_sk <= SPREAD
        B_f = R.bound_objective(X, y, C, c["reg_C"], ref["theta"])
        assert f_ref <= f_host + 4 * B_f and f_ref <= f_sk + 4 * B_f         # the optimum cannot lose: beyond rounding never above


@pytest.mark.parametrize("name", R.IDS)
def test_every_test_table_converges_with_headroom_under_the_iteration_bound(name):
    """The reference solve and the device's iteration restated (lr_ref.newton_cg) both stop within a quarter of
    DVAE_LR_MAX_ITERATIONS on every table of tests/test_gpu_lr.py: no GPU case can sit at the bound."""
    c = R.case(name)
    S = c["S"]
    for q, C in enumerate(c["classes"]):
        ref = c["problems"][q]
        theta, _f, gmax, its, n_eval, n_cg = R.newton_cg(c["X"][:S], c["labels"][q, :S], C, c["reg_C"], 1e-8)
        print("%s[%d]: reference %d Newton steps to %.1e; the device's iteration restated: %d steps, %d evaluations, %d conjugate-gradient steps"
              % (name, q, ref["iterations"], ref["gmax"], its, n_eval, n_cg))
        assert 0 <= ref["iterations"] and 4 * ref["iterations"] <= _lrlib.MAX_ITERATIONS and ref["gmax"] <= 1e-13
        assert 0 <= its and 4 * its <= _lrlib.MAX_ITERATIONS and gmax <= 1e-8
        assert n_cg <= its * _lrlib.MAX_CG and n_eval <= its + 1 + 4           # hardly a halving
        H = R.hessian(c["X"][:S], c["labels"][q, :S], C, c["reg_C"], ref["theta"])
        assert float(np.abs(R.centred(theta, C, c["D"]) - ref["theta"]).max()) <= 2.0 * R.pinv_norm(H, C, c["D"]) * 1.1e-8


# ---- 3. InfoE -----------------------------------------------------------------------------------------------------------------------
def test_infoe_from_log_loss():
    per, score = E.infoe_from_log_loss([0.5, 0.0, 1.2, 0.25], [1.0, 2.0, 1.0, 0.5])
    assert per.tolist() == [0.5, 1.0, 1.0 - 1.2, 0.5] and score == pytest.approx((0.5 + 1.0 + 0.0 + 0.5) / 4, abs=1e-16)     # clipped in the mean only
    per, score = E.infoe_from_log_loss([0.0, 0.3], [0.0, 0.6])              # a one-class factor: no entropy, NaN, left out of the mean
    assert np.isnan(per[0]) and per[1] == 0.5 and score == 0.5
    per, score = E.infoe_from_log_loss([float("nan"), float("inf"), 0.1], [1.0, 1.0, float("nan")])    # no counted row: 0 / 0
    assert np.isnan(per).all() and np.isnan(score)
    per, score = E.infoe_from_log_loss([], [])
    assert per.shape == (0,) and np.isnan(score)
    per, score = E.infoe_from_log_loss([2.0], [1.0])                        # worse than the frequencies: negative per factor, 0 in the mean
    assert per.tolist() == [-1.0] and score == 0.0
    for a, b in (([0.1], [0.5, 0.5]), ([[0.1]], [[0.5]]), (0.1, 0.5)):
        with pytest.raises(ValueError, match="two \\[K\\] vectors"):
            E.infoe_from_log_loss(a, b)
    for args in (([0.5, 0.0, 1.2], [1.0, 0.0, 1.0]), ([0.3], [0.6])):
        mine, theirs = E.infoe_from_log_loss(*args), R.infoe(*args)
        assert mine[0].tobytes() == theirs[0].tobytes() and mine[1] == theirs[1]


def test_thresholds_of_the_end_to_end_gpu_test_on_the_restatement_alone():
    rows = SR.end_to_end_rows()
    got = {name: R.infoe_reference(tab, SR.GRID, rows[:240], rows[240:]) for name, tab in SR.end_to_end_tables().items()}
    print({k: (round(v["infoe_train"], 6), round(v["infoe_test"], 6)) for k, v in got.items()})
    for key in ("infoe_train", "infoe_test"):
        assert got["ideal"][key] > got["rotated"][key] + 1e-3 > got["collapsed"][key] + 0.5
    for v in got.values():
        assert (v["infoe_train_per_factor"] >= 0.0).all()                    # theta = (0, log frequencies) is feasible at no penalty
        assert np.abs(v["ce_null_train"] - [-(p * np.log(p)).sum() for p in ([1 / 3] * 3, [1 / 4] * 4, [1 / 5] * 5, [1 / 6] * 6)]).max() < 0.02
    raw = {name: R.infoe_reference(tab, SR.GRID, rows[:240], rows[240:], standardize=False) for name, tab in SR.end_to_end_tables().items()}
    assert abs(raw["ideal"]["infoe_train"] - raw["rotated"]["infoe_train"]) <= 1e-9      # a linear probe does not see a rotation


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
    monkeypatch.setattr(_lrlib, "lib", no_library)
    mean = torch.zeros(6, 4)
    ok = dict(n_train=4, n_test=2)
    for sizes, kw, msg in (([3, 3], ok, "does not enumerate"), ([3, 2], dict(n_train=0, n_test=2), r"n_train must lie in \[1, "),
                           ([3, 2], dict(n_train=4, n_test=0), "n_test must be at least 1"), ([3, 2], dict(n_train=4, n_test=3), "n_train \\+ n_test must be at most 6"),
                           ([3, 2], {}, "n_train \\+ n_test must be at most 6"), ([0, 2], ok, "positive sizes"),
                           ([3, 2], dict(ok, C=0.0), "C must be a positive finite number"), ([3, 2], dict(ok, C=float("inf")), "C must be a positive"),
                           ([3, 2], dict(ok, C=float("nan")), "C must be a positive"), ([3, 2], dict(ok, C="1"), "C must be a positive"),
                           ([3, 2], dict(ok, rows=[0, 1, 2, 3, 4, 6]), r"in \[0, 6\)"), ([3, 2], dict(ok, rows=[0, 1, 2]), "rows must hold n_train \\+ n_test = 6")):
        with pytest.raises(ValueError, match=msg):
            E.infoe_from_table(mean, sizes, **kw)
    with pytest.raises(ValueError, match="between 1 and 8"):                # nine factors
        E.infoe_from_table(torch.zeros(512, 2), [2] * 9, n_train=10, n_test=5)
    with pytest.raises(ValueError, match="between 1 and 64 latent dimensions"):      # (the limit of dci_from_table's checks is the same)
        E.infoe_from_table(torch.zeros(6, 65), [3, 2], **ok)
    with pytest.raises(ValueError, match="table"):
        E.infoe_from_table(torch.zeros(6), [3, 2], **ok)
    bad = mean.clone()
    bad[4, 1] = float("nan")
    with pytest.raises(ValueError, match="NaN or an infinity"):
        E.infoe_from_table(bad, [3, 2], **ok)
    with pytest.raises(_lib.DvaeHipError, match="no CPU"):
        E.infoe_from_table(mean, [3, 2], **ok)
    # fit = "device" of the two scores that had the host fit alone: the value and the library's limits, before any device work
    for fn, kw in ((E.explicitness_from_table, ok), (E.factor_scores_from_table, dict(n_train=4, n_eval=2, batch_size=2))):
        with pytest.raises(ValueError, match='fit must be "host" or "device"'):
            fn(mean, [3, 2], fit="gpu", **kw)
        with pytest.raises(ValueError, match="between 1 and 64 (features|latent dimensions)"):
            fn(torch.zeros(6, 65), [3, 2], fit="device", **kw)
        with pytest.raises(_lib.DvaeHipError, match="no CPU"):
            fn(mean, [3, 2], fit="device", **kw)
    with pytest.raises(ValueError, match="between 1 and 8"):
        E.explicitness_from_table(torch.zeros(512, 2), [2] * 9, n_train=10, n_test=5, fit="device")
    with pytest.raises(ValueError, match="fit between 1 and 16384 rows"):
        E.factor_scores_from_table(mean, [3, 2], n_train=16385, n_eval=2, batch_size=2, fit="device")
    # fit_logistic_regression_device
    x, y = torch.zeros(5, 3), torch.tensor([0, 1, 2, 1, 0])
    for args, kw, msg in (((torch.zeros(5), y, 3), {}, r"\[n, D\] matrix"), ((torch.zeros(16385, 1), torch.zeros(16385), 2), {}, "between 1 and 16384 rows"),
                          ((torch.zeros(5, 65), y, 3), {}, "between 1 and 64 features"), ((x, y, 257), {}, "between 1 and 256"),
                          ((x, y, 0), {}, "between 1 and 256"), ((x, y, 2), {}, r"labels must hold 5 classes in \[0, 2\)"),
                          ((x, y[:4], 3), {}, "labels must hold 5 classes"), ((x, y, 3), dict(C=0.0), "C must be a positive finite"),
                          ((x, y, 3), dict(tolerance_grad=-1.0), "tolerance_grad must be a finite number >= 0"),
                          ((x, y, 3), dict(tolerance_grad=float("nan")), "tolerance_grad must be"),
                          ((torch.full((5, 3), float("inf")), y, 3), {}, "NaN or an infinity")):
        with pytest.raises(ValueError, match=msg):
            E.fit_logistic_regression_device(*args, **kw)
    with pytest.raises(_lib.DvaeHipError, match="no CPU"):
        E.fit_logistic_regression_device(x, y, 3)
    model = _Model().train()
    ev = E.Evaluator(model, None, is_progress_bar=False)
    with pytest.raises(ValueError, match="known true factors"):
        ev.compute_infoe(_Loader([0, 1, 2], None))
    for kw, msg in ((dict(n_train=0), "n_train must lie"), (dict(n_train=5, n_test=2), "n_train \\+ n_test must be at most 6"), (dict(ok, C=-1.0), "C must be")):
        with pytest.raises(ValueError, match=msg):
            ev.compute_infoe(_Loader(_Factors(6), None), **kw)
    with pytest.raises(ValueError, match='fit must be "host" or "device"'):
        ev.compute_explicitness(_Loader(_Factors(6), None), fit="x", **ok)
    with pytest.raises(ValueError, match='fit must be "host" or "device"'):
        ev.compute_factor_scores(_Loader(_Factors(6), None), n_train=4, n_eval=2, batch_size=2, fit="x")
    with pytest.raises(ValueError, match=r"data set of 5 images does not enumerate lat_sizes=\[3, 2\]"):
        ev.compute_infoe(_Loader(_Factors(5), None), **ok)
    assert model.modes == [] and model.training
    loader = _Loader(_Factors(6), [(torch.rand(4, 1), None), (torch.rand(2, 1), None)])
    with pytest.raises(_lib.DvaeHipError, match="no CPU"):                 # valid arguments: the table is on the CPU
        ev.compute_infoe(loader, **ok)
    assert model.modes == [False, False] and model.training               # encoded in eval mode, and the mode is as it was


def test_call_writes_infoe_on_request(monkeypatch, tmp_path):
    seen = []
    model = _Model().train()
    ev = E.Evaluator(model, None, is_progress_bar=False, save_dir=str(tmp_path))
    result = {"infoe_train": 0.75, "infoe_test": 0.5, "infoe_train_per_factor": np.array([0.75, np.nan]), "report": np.zeros((2, 4)),
              "n_unseen": np.array([0, 1]), "n_train": 4, "n_test": 2, "C": 1.0, "standardize": True}
    monkeypatch.setattr(ev, "compute_infoe", lambda loader, **kw: seen.append((loader, kw, model.training)) or result)
    monkeypatch.setattr(ev, "compute_losses", lambda loader: {"loss": 1.5})
    loader = object()
    assert ev(loader) == (None, {"loss": 1.5}) and seen == [] and os.listdir(tmp_path) == ["test_losses.log"]
    assert ev(loader, is_losses=False, is_infoe=True) == (None, None)
    assert seen == [(loader, {}, False)] and model.training
    assert ev(loader, is_losses=False, is_infoe=True, infoe_args=dict(n_train=4, n_test=2, C=2.0)) == (None, None)
    assert seen[-1] == (loader, dict(n_train=4, n_test=2, C=2.0), False)
    assert E.INFOE_FILE == "infoe.log" and sorted(os.listdir(tmp_path)) == ["infoe.log", "test_losses.log"]
    logged = json.load(open(tmp_path / "infoe.log"))
    assert set(logged) == set(result) - {"report"} and logged["infoe_train"] == 0.75 and logged["n_unseen"] == [0, 1]
    assert logged["infoe_train_per_factor"][0] == 0.75 and np.isnan(logged["infoe_train_per_factor"][1])
