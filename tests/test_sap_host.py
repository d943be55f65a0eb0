"""CPU: the host side of the discrete-factor SAP score -- the thirteenth library's C-ABI (include/dvae_sap_hip.h ==
disvae_amd/_saplib.py == the built lib_more/libdvae_sap_hip.so), its row of build.py's MORE_TARGETS (the other four lists, the 31
sources, the eleven libraries of lib/ and the one of lib/ext/ untouched), the rules its source obeys, the refusal of bad arguments
before any launch, the restatement tests/sap_ref.py against the installed scikit-learn, the prediction rule, the score from
hand-made score matrices, and the argument errors of the public functions before any device work.

Measured here (scikit-learn 1.7.2; the tables of TABLES below, C = 0.01):
    |w|, |b| of the restatement against LinearSVC(tol=1e-10, max_iter=200000): at most 7.19e-8 (the sharp table)  -> THETA_TOL = 7.2e-7
    its objective against that LinearSVC's: never above it by more than 4e-16 of its value
    predictions of the two: identical on every training row of every table
    sap_discrete of the restatement against disentanglement_lib's loop with default LinearSVC fits (tol=1e-4): 0 apart, every entry
    of the three score matrices equal (0.236349 sharp, 0.072368 noisy, 0.003618 noise).  Ten times nothing allows nothing, and an
    entry moves in steps of 1 / 1520 test rows when the default fit's looser stop flips a row   -> SAP_TOL = 10 / 1520 = 6.6e-3
    That is more than the score of the noise table, so every ENTRY is held too, to a margin derived for it: with delta the largest
    coefficient difference between the default fit and ours (4.2e-5 sharp, 9.4e-6 noisy, 1.0e-5 noise) a decision value moves by at
    most delta (|x| + 1), so only a test row whose top two decision values lie within 2 delta (|x| + 1) can be predicted differently:
    at most 63, 87 and 16 of the 1 520 rows in an entry of the three tables (the 40-class factor, whose decision lines nearly coincide).
    Newton steps: at most 7; halvings of a step: none on any table here -- columns drawn from a continuous distribution never take
    one; the dyadic hinge table of sap_ref.py, whose optimum has rows exactly on the hinge, takes all of them.
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

import sap_ref as R
import disvae_amd
from disvae_amd import _cabi, _infolib, _lib, _masslib, _saplib
from disvae_amd import evaluate as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dvae_sap_hip.h")
CSRC = os.path.join(ROOT, "disentangling-vae_amd", "csrc")
SOURCE = "svm_1d.hip"
DUMMY = 1 << 20                                                   # aligned non-NULL address, never dereferenced
SAP_TOL = 10.0 / 1520                                             # ten test rows of one entry (measured: 0; the module docstring)
THETA_TOL = 7.2e-7                                                # 10 x the worst measured against the tight LinearSVC
SIZES = (3, 6, 40, 16)                                            # 11 520 rows: 10 000 to fit
# (name, family, lat_sizes, training rows, test rows, seed)
TABLES = [("sharp-10000", "sharp", SIZES, 10000, 1520, 1), ("noisy-10000", "noisy", SIZES, 10000, 1520, 1),
          ("noise-10000", "noise", SIZES, 10000, 1520, 1), ("two-classes-7", "noisy", (2, 5, 4), 7, 7, 2),
          ("constant-30", "constant", (3, 4, 5), 30, 30, 3), ("absent-class-30", "noisy", (3, 20), 30, 30, 4)]


def _build():
    spec = importlib.util.spec_from_file_location("dvae_build_sap", os.path.join(ROOT, "disentangling-vae_amd", "build.py"))
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
    declared = sorted(set(re.findall(r"\b(dvae_sap_[a-zA-Z0-9_]+)\s*\(", _header())))
    assert declared == sorted(_saplib.SIGNATURES)
    assert declared == sorted(["dvae_sap_version", "dvae_sap_last_error", "dvae_sap_problems", "dvae_sap_fit", "dvae_sap_accuracy"])
    exported = sorted(set(re.findall(r" T (dvae_\w+)", _nm(os.path.abspath(_saplib.LIB_PATH), "-D", "--defined-only"))))
    assert exported == declared
    assert re.findall(r" U (dvae_\w+)", _nm(os.path.abspath(_saplib.LIB_PATH), "-D")) == []
    kinds = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_long: "l", ctypes.c_double: "d"}
    for name, params in re.findall(r"\b(dvae_sap_[a-zA-Z0-9_]+)\s*\(([^)]*)\)", _header()):
        got = []
        for prm in [x.strip() for x in params.split(",") if x.strip() != "void"]:
            got.append("p" if "*" in prm else ("l" if prm.startswith("long") else "d" if prm.startswith("double") else "i"))
        assert got == [kinds[t] for t in _saplib.SIGNATURES[name]], name
    macros = {k: int(v) for k, v in re.findall(r"#define (DVAE_SAP_\w+) (\d+)", _header())}
    mirrored = {"DVAE_SAP_VERSION": _saplib.VERSION, "DVAE_SAP_MAX_FACTORS": _saplib.MAX_FACTORS, "DVAE_SAP_MAX_CLASSES": _saplib.MAX_CLASSES,
                "DVAE_SAP_MAX_D": _saplib.MAX_D, "DVAE_SAP_THREADS": _saplib.THREADS, "DVAE_SAP_MAX_ROWS": _saplib.MAX_ROWS,
                "DVAE_SAP_MAX_ITERATIONS": _saplib.MAX_ITERATIONS, "DVAE_SAP_MAX_HALVINGS": _saplib.MAX_HALVINGS}
    assert macros == mirrored                                            # every macro of the header, none besides
    assert (R.MAX_ITERATIONS, R.MAX_HALVINGS) == (_saplib.MAX_ITERATIONS, _saplib.MAX_HALVINGS)
    # the limits: DCI's 10 240 rows fit the LDS, Cars3D's 183-valued factor is accepted, eight factors
    assert _saplib.MAX_ROWS >= 10240 and _saplib.MAX_CLASSES >= 256 and _saplib.MAX_FACTORS == _infolib.MAX_FACTORS == 8
    assert 5 * _saplib.MAX_ROWS + 1024 <= 160 * 1024
    assert _saplib.lib().dvae_sap_version() == _saplib.VERSION == 1
    binding = open(_saplib.__file__).read()
    assert 'Binding.for_library("sap", SIGNATURES, _RESTYPE' in binding and "LIB_PATH = _binding.path" in binding
    assert _saplib._binding.last_error == "dvae_sap_last_error" and _saplib._binding.signatures is _saplib.SIGNATURES
    assert _saplib._binding.soname == "libdvae_sap_hip.so"
    monkeypatch.setenv("DVAE_SAP_HIP_LIB", "/elsewhere/lib.so")            # the override, read when a binding is made
    assert _cabi.Binding.for_library("sap", {}, {}, "", subdir=os.path.join("..", "lib_more")).path == "/elsewhere/lib.so"
    monkeypatch.delenv("DVAE_SAP_HIP_LIB")
    assert os.path.normpath(_saplib.LIB_PATH).endswith(os.path.join("disentangling-vae_amd", "lib_more", "libdvae_sap_hip.so"))
    assert os.path.normpath(_masslib.LIB_PATH).endswith(os.path.join("lib", "ext", "libdvae_mass_hip.so"))      # as before
    for name in ("sap_discrete_from_table", "sap_discrete_from_score_matrix"):
        assert name in disvae_amd.__all__ and getattr(disvae_amd, name) is getattr(E, name)


def test_build_has_the_fifth_list_and_the_other_four_are_unchanged():
    build = _build()
    assert [tuple(row) for row in build.MORE_TARGETS] == [("sap", ["svm_1d"], "dvae_sap_hip.h")]
    assert [tuple(row) for row in build.EXTRA_TARGETS] == [("mass", ["posterior_mass"], "dvae_mass_hip.h")]
    assert [tuple(row) for row in build.SCORE_PLUGIN_TARGETS] == [("sep", ["latent_loo"], "dvae_sep_hip.h")]
    assert [tuple(row) for row in build.PLUGIN_TARGETS] == [("mmd", ["mmd_pairs"], "dvae_mmd_hip.h")]
    assert [n for n, _s, _h in build.TARGETS] == ["", "eval", "score", "info", "irs", "unsup", "udr", "dci", "dip"]
    assert "svm_1d" not in build.ALL_SOURCES and len(build.ALL_SOURCES) == 31
    assert "svm_1d" not in open(os.path.join(ROOT, "tools", "isa_identity.py")).read()
    assert build.SAP_SOURCES == ["svm_1d"] and os.path.exists(os.path.join(build.SRC, SOURCE))
    pkg = os.path.join(ROOT, "disentangling-vae_amd")
    assert os.path.abspath(build.SAP_LIB) == os.path.join(pkg, "lib_more", "libdvae_sap_hip.so") and os.path.exists(build.SAP_LIB)
    assert os.path.abspath(build.SAP_LIB) == os.path.abspath(_saplib.LIB_PATH)
    assert os.path.abspath(build.MASS_LIB) == os.path.join(pkg, "lib", "ext", "libdvae_mass_hip.so")
    assert sorted(os.path.basename(h) for h in build.SAP_HEADERS if "include" in h.split(os.sep)) == ["dvae_hip.h", "dvae_sap_hip.h"]
    assert build._target(*build.MORE_TARGETS[0], subdir=build.MORE_DIR)[3] == os.path.join(build.OBJ, "flags_sap.txt")
    assert open(os.path.join(build.OBJ, "flags_sap.txt")).read() == open(os.path.join(build.OBJ, "flags_sep.txt")).read().replace(
        "latent_loo", "svm_1d")                                           # build() stamped it: the same flags and stamp logic
    inside = [f for d, _dirs, files in os.walk(os.path.join(pkg, "lib")) for f in files if re.fullmatch(r"libdvae(_\w+)?_hip\.so", f)]
    assert len(inside) == 12 and "libdvae_sap_hip.so" not in inside
    assert [f for f in os.listdir(os.path.join(pkg, "lib_more")) if f.endswith(".so")] == ["libdvae_sap_hip.so"]
    ignored = subprocess.run(["git", "check-ignore", "-q", build.SAP_LIB], cwd=ROOT).returncode
    assert ignored in (0, 128)                                            # ignored like lib/ (128: not a git checkout)
    text = open(os.path.join(pkg, "build.py")).read()
    assert len(re.findall(r"\b_build_target\(", text)) == 2               # one helper for all five lists
    src = open(os.path.join(CSRC, SOURCE)).read()
    assert sorted(re.findall(r'^#include "([^"]+)"', src, re.M)) == ["../../include/dvae_sap_hip.h", "common.h", "last_error.h"]


def test_source_obeys_the_rules_of_the_score_libraries():
    src = open(os.path.join(CSRC, SOURCE)).read()
    assert len(re.findall(r'^#include "last_error\.h"', src, re.M)) == 1
    assert not re.search(r"\bthread_local\b", src) and not re.search(r"^void set_error\(", src, re.M)
    for name in ("put_f64", "get_f64", "chunks_of", "lesser"):              # table_stats.h is their one home
        assert not re.search(r"^[ \w]*\b(?:void|double|int|T)\s+%s\s*\([^;{]*\)\s*\{" % name, src, re.M), name
    code = re.sub(r"//[^\n]*", "", src.split("#include", 1)[1])
    assert not re.search(r"atomic", code)                                   # no atomics of any kind
    assert "while" not in code and "hipLaunchCooperativeKernel" not in src  # bounded loops only, no cooperative launch
    assert not re.search(r"hipMalloc|hipFree|hipMemcpy|hipMemset|Synchronize", src)    # the entry points only enqueue
    assert len(re.findall(r"^#pragma clang fp contract\(off\)$", src, re.M)) == 1        # no fused multiply-add in the decision value
    assert "fma(" not in code
    for bound in ("it <= DVAE_SAP_MAX_ITERATIONS", "hv <= DVAE_SAP_MAX_HALVINGS"):
        assert bound in code


def _put(good, i, v):
    return good[:i] + [v] + good[i + 1:]


def test_bad_arguments_are_refused_before_a_launch_with_the_librarys_own_text():
    h = _saplib.lib()
    assert h is _saplib.lib()                                              # loaded once
    cls = _saplib.host_classes([3, 2])
    #      table  rows   labels n_cls N  D  K  S  C     coef   iters  stream
    fit = [DUMMY, DUMMY, DUMMY, cls, 6, 3, 2, 4, 0.01, DUMMY, DUMMY, None]
    #      table  rows   labels n_cls N  D  K  T  coef   correct pred stream
    acc = [DUMMY, DUMMY, DUMMY, cls, 6, 3, 2, 4, DUMMY, DUMMY, None, None]
    bad_fit = [_put(fit, i, None) for i in (0, 1, 2, 3, 9, 10)]
    bad_fit += [_put(fit, 4, 0), _put(fit, 4, 2 ** 31), _put(fit, 5, 0), _put(fit, 5, _saplib.MAX_D + 1), _put(fit, 6, 0),
                _put(fit, 6, _saplib.MAX_FACTORS + 1), _put(fit, 7, 0), _put(fit, 7, _saplib.MAX_ROWS + 1), _put(fit, 8, 0.0),
                _put(fit, 8, -1.0), _put(fit, 8, float("inf")), _put(fit, 8, float("nan")),
                _put(fit, 3, _saplib.host_classes([3, 0])), _put(fit, 3, _saplib.host_classes([_saplib.MAX_CLASSES + 1, 2]))]
    bad_acc = [_put(acc, i, None) for i in (0, 1, 2, 3, 8, 9)]
    bad_acc += [_put(acc, 4, 0), _put(acc, 5, 0), _put(acc, 6, 9), _put(acc, 7, 0), _put(acc, 7, 2 ** 31),
                _put(acc, 3, _saplib.host_classes([3, -1]))]
    for name, cases in (("dvae_sap_fit", bad_fit), ("dvae_sap_accuracy", bad_acc)):
        for args in cases:
            with pytest.raises(_lib.DvaeHipError) as e:
                _saplib.call(name, *args)
            own = h.dvae_sap_last_error().decode()
            assert "invalid argument" in own and SOURCE in own, (args, own)
            assert str(e.value) == "%s failed (-1): %s" % (name, own)
    with pytest.raises(_lib.DvaeHipError, match=r"S >= 1 && S <= DVAE_SAP_MAX_ROWS"):      # the row limit, in the library's own words
        _saplib.call("dvae_sap_fit", *_put(fit, 7, _saplib.MAX_ROWS + 1))
    assert SOURCE not in _infolib.lib().dvae_info_last_error().decode()    # every library keeps its own buffer
    # factors of one class have no problem: nothing to fit, nothing is launched and no output pointer is needed
    one = _saplib.host_classes([1, 1])
    assert h.dvae_sap_fit(DUMMY, DUMMY, DUMMY, one, 6, 3, 2, 4, 0.01, None, None, None) == 0
    for classes, want in (([3, 2], 4), ([1], 0), ([2], 1), ([3, 6, 40, 32, 32], 113), ([4, 24, 183], 211), ([1, 2, 3], 4)):
        assert h.dvae_sap_problems(_saplib.host_classes(classes), len(classes)) == _saplib.problems(classes) == want == len(R.problem_list(classes))
    for classes in ([], [0], [257], [2] * 9):
        assert _saplib.problems(classes) == -1 and (not classes or h.dvae_sap_problems(_saplib.host_classes(classes), len(classes)) == -1)


def test_call_loads_through_the_modules_lib(monkeypatch):
    class Boom(Exception):
        pass

    def boom():
        raise Boom("lib() of the module was asked")
    monkeypatch.setattr(_saplib, "lib", boom)
    with pytest.raises(Boom, match="was asked"):
        _saplib.call("dvae_sap_version")


# ---- 2. the restatement against scikit-learn -------------------------------------------------------------------------------------
def _split(family, sizes, S, T, seed):
    tab = R.table(family, sizes, len(sizes), seed=seed)
    perm = np.random.default_rng(seed).permutation(tab.shape[0])
    return tab, perm[:S], perm[S:S + T]


@pytest.mark.parametrize("name,family,sizes,S,T,seed", TABLES, ids=[t[0] for t in TABLES])
def test_restatement_against_linear_svc(name, family, sizes, S, T, seed):
    svm = pytest.importorskip("sklearn.svm")
    tab, train, test = _split(family, sizes, S, T, seed)
    lt, _le, n = R.labels_of(train, train, sizes)
    if name.startswith("absent"):
        assert n[1] < sizes[1]                                            # a value of the factor that no training row carries
    if name.startswith("two"):
        assert n[0] == 2
    coef, its, halvings = R.fit(tab, train, lt, n, 0.01)
    assert (its >= 1).all() and its.max() <= 9
    worst_theta, worst_f, mismatches, close, fitted = 0.0, -np.inf, 0, 0, 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for d in range(len(sizes)):
            x, p0 = tab[train, d].astype(np.float64), 0
            for j, Cj in enumerate(n):
                npb = R.problems_of(Cj)
                if Cj >= 2 and (j == d or d == 0):                       # the latent of the factor, and latent 0 against every factor
                    clf = svm.LinearSVC(C=0.01, class_weight="balanced", tol=1e-10, max_iter=200000).fit(x[:, None], lt[j])
                    theirs = np.column_stack([clf.coef_[:, 0], clf.intercept_])
                    ours = coef[d, p0:p0 + npb]
                    assert theirs.shape == ours.shape
                    worst_theta = max(worst_theta, float(np.abs(theirs - ours).max()))
                    for p, (_j, k) in enumerate(R.problem_list([Cj])):
                        pos = lt[j] == k
                        cp, cn = R.weights(pos, Cj, 0.01)
                        f_ours, f_theirs = R.objective(x, pos, cp, cn, *ours[p]), R.objective(x, pos, cp, cn, *theirs[p])
                        worst_f = max(worst_f, (f_ours - f_theirs) / f_theirs)
                    mine, other = R.predict(ours, x, Cj), clf.predict(x[:, None])
                    differ = mine != other
                    if differ.any():                                      # allowed only where the top two decision values are that close
                        top = np.sort(R.decisions(ours, x), axis=1)[:, -2:] if Cj >= 3 else np.stack([np.zeros(len(x)), R.decisions(ours, x)[:, 0]], axis=1)
                        tight = np.abs(top[:, 1] - top[:, 0]) < THETA_TOL * (np.abs(x) + 1.0)
                        assert tight[differ].all()
                        close += int(differ.sum())
                    mismatches += int(differ.sum())
                    fitted += npb
                p0 += npb
    print("%s: %d problems, worst |d theta| %.3e (allowed %.1e), objective at most %.2e of its value above LinearSVC's, %d of %d rows "
          "predicted differently, at most %d Newton steps, %d halvings" % (name, fitted, worst_theta, THETA_TOL, worst_f, mismatches, S,
                                                                          its.max(), halvings.sum()))
    assert worst_f <= 4 * (S + 2) * R.U                                 # the exact minimiser cannot lose: beyond rounding never above
    assert worst_theta <= THETA_TOL
    assert close <= 0.01 * S


@pytest.mark.parametrize("name,family,sizes,S,T,seed", TABLES[:3], ids=[t[0] for t in TABLES[:3]])
def test_sap_against_the_loop_of_disentanglement_lib(name, family, sizes, S, T, seed):
    """sap_score.py's discrete branch restated with default LinearSVC fits: score_matrix[i, j] = mean(predict(mu_i_test) == y_j_test)."""
    svm = pytest.importorskip("sklearn.svm")
    tab, train, test = _split(family, sizes, S, T, seed)
    ours = R.reference(tab, sizes, train, test)
    v_train, v_test = R.factor_values(train, sizes), R.factor_values(test, sizes)
    _lt, _le, n = R.labels_of(train, test, sizes)
    assert n == list(sizes)                                               # every value is seen in training: ranks are values
    theirs, may_flip = np.zeros((len(sizes), len(sizes))), np.zeros((len(sizes), len(sizes)))
    worst_delta = 0.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i in range(len(sizes)):
            x, p0 = tab[test, i].astype(np.float64), 0
            for j, Cj in enumerate(n):
                clf = svm.LinearSVC(C=0.01, class_weight="balanced").fit(tab[train, i].astype(np.float64)[:, None], v_train[j])
                theirs[i, j] = np.mean(clf.predict(x[:, None]) == v_test[j])
                mine = ours["coef"][i, p0:p0 + R.problems_of(Cj)]
                p0 += R.problems_of(Cj)
                delta = float(np.abs(np.column_stack([clf.coef_[:, 0], clf.intercept_]) - mine).max())
                dec = np.sort(R.decisions(mine, x), axis=1)
                gap = dec[:, -1] - dec[:, -2] if Cj >= 3 else np.abs(dec[:, 0])
                may_flip[i, j] = (gap <= 2.0 * delta * (np.abs(x) + 1.0)).sum()
                worst_delta = max(worst_delta, delta)
    apart = np.abs(ours["score_matrix"] - theirs) * len(test)
    print("%s: sap_discrete %.6f, disentanglement_lib's loop %.6f (allowed %.1e apart); entries at most %g test rows apart, at most %g rows may "
          "flip in an entry; default fits within %.2e of ours" % (name, ours["sap_discrete"], R.sap(theirs), SAP_TOL, apart.max(),
                                                                  may_flip.max(), worst_delta))
    assert (apart <= may_flip + 1e-9).all()                               # entry by entry: only rows that close to a boundary may differ
    assert abs(ours["sap_discrete"] - R.sap(theirs)) <= SAP_TOL
    assert E.sap_discrete_from_score_matrix(theirs) == R.sap(theirs)


def test_a_row_exactly_on_the_hinge_takes_every_halving_and_keeps_the_minimiser():
    """The hinge table: the optimum of class 0 is (-3 / 11, -1 / 11), where both positives have s (w x + b) = 1.  The minimisers of the
    two pieces that meet there are one point in exact arithmetic and two neighbours in fp64; the full step hops between them, no
    halving of it lowers the objective, and the iteration leaves through the exit that keeps the current point."""
    tab = R.table("hinge", (3, 2), 1)
    train = np.array(R.HINGE_ROWS)
    lt, _le, n = R.labels_of(train, train, (3, 2))
    assert n == [3, 2] and lt[0].tolist() == [0, 1, 0, 1, 2] and tab[train, 0].tolist() == [-4.0, 3.0, -4.0, 4.0, 4.0]
    for rep, C in ((1, 0.5), (60, 0.5 / 60)):                              # the same objective on 5 and on 300 rows
        x, pos = np.tile(tab[train, 0].astype(np.float64), rep), np.tile(lt[0] == 0, rep)
        w, b, its, halvings = R.newton(x, pos, 3, C)
        cp, cn = R.weights(pos, 3, C)
        B, normH = R.bound(x, pos, cp, cn, w, b)
        assert halvings == R.MAX_HALVINGS + 1 and 1 <= its <= 6
        assert abs(w + 3.0 / 11.0) <= B and abs(b + 1.0 / 11.0) <= B and R.near_hinge(x, pos, w, b, B)
        assert np.abs(R.gradient(x, pos, cp, cn, w, b)).max() <= B * normH
        assert R.newton(x, lt.repeat(rep, axis=1)[0] == 1, 3, C)[3] == 0   # the other classes of the table take none


# ---- 3. the prediction rule and the score ----------------------------------------------------------------------------------------
def test_prediction_rule():
    x = np.array([-2.0, 0.0, 0.5, 3.0])
    wb = np.array([[1.0, 0.0], [1.0, 0.0], [2.0, -1.0]])                   # classes 0 and 1 tie everywhere; class 2 wins above x = 1
    assert R.predict(wb, x, 3).tolist() == [0, 0, 0, 2]                    # ties: the lowest class
    assert R.predict(np.array([[0.0, 0.0]] * 5), x, 5).tolist() == [0, 0, 0, 0]
    assert R.predict(np.array([[1.0, 0.0]]), x, 2).tolist() == [0, 0, 1, 1]       # the sign test: 0 is not > 0
    assert R.predict(np.zeros((0, 2)), x, 1).tolist() == [0, 0, 0, 0]      # one class present: that class
    # the product is rounded before the sum: a fused multiply-add would give another sign here
    w, xv = 1.0 + 2.0 ** -30, np.array([1.0 + 2.0 ** -30])
    b = -float(np.float64(w) * xv[0])
    assert R.decisions(np.array([[w, b]]), xv)[0, 0] == 0.0 and R.predict(np.array([[w, b]]), xv, 2).tolist() == [0]
    # a test row whose value no training row carries counts as an error
    tab = R.table("sharp", (3, 4), 1, seed=0)
    train, test = np.array([0, 1, 4, 5, 8, 9]), np.arange(12)              # factor 1: values 0 and 1 only
    lt, le, n = R.labels_of(train, test, (3, 4))
    assert n == [3, 2] and le[1].tolist() == [0, 1, -1, -1] * 3 and lt.dtype == le.dtype == np.int32
    coef, its, _hv = R.fit(tab, train, lt, n, 0.01)
    correct, predicted = R.accuracy(tab, test, le, n, coef)
    assert coef.shape == (1, 4, 2) and predicted.shape == (1, 2, 12) and predicted.min() >= 0
    assert correct[0, 1] == (predicted[0, 1] == le[1]).sum() <= 6
    assert R.problem_list([3, 2, 1]) == [(0, 0), (0, 1), (0, 2), (1, 1)]


def test_score_from_ideal_rotated_and_collapsed_matrices():
    ideal = np.array([[1.0, 0.2, 0.1], [0.3, 0.9, 0.1], [0.3, 0.2, 0.8], [0.3, 0.2, 0.1]])
    assert E.sap_discrete_from_score_matrix(ideal) == pytest.approx(((1.0 - 0.3) + (0.9 - 0.2) + (0.8 - 0.1)) / 3, abs=1e-15)
    rotated = np.array([[0.6, 0.5], [0.6, 0.5], [0.1, 0.5]])                # two latents hold every factor alike: no gap
    assert E.sap_discrete_from_score_matrix(rotated) == 0.0
    collapsed = np.full((5, 3), 1.0 / 3.0)                                 # every latent guesses
    assert E.sap_discrete_from_score_matrix(collapsed) == 0.0
    assert E.sap_discrete_from_score_matrix([[0.7, 0.4]]) == pytest.approx(0.55, abs=1e-15)       # one latent: the runner-up is 0
    for m in (ideal, rotated, collapsed, np.array([[0.7, 0.4]])):
        assert E.sap_discrete_from_score_matrix(m) == R.sap(m)
        assert np.array_equal(E.largest_gap(m), np.sort(m, axis=0)[::-1][0] - (np.sort(m, axis=0)[::-1][1] if len(m) > 1 else 0.0))
    for bad in (np.zeros(3), np.zeros((0, 3)), np.zeros((2, 2, 2))):
        with pytest.raises(ValueError, match=r"score_matrix must be a non-empty \[D, K\] matrix"):
            E.sap_discrete_from_score_matrix(bad)
    # information_scores_from_statistics uses the same gap, as before
    counts = np.array([[5, 0, 0, 5], [3, 2, 2, 3]])
    got = E.information_scores_from_statistics(counts, (2,), 2, [1.0, 1.0], [0.25], [[0.5], [0.1]])
    assert got["sap_continuous"] == pytest.approx(1.0 - 0.04, abs=1e-15)


def test_thresholds_of_the_end_to_end_gpu_test_on_the_restatement_alone():
    rows = R.end_to_end_rows()
    got = {}
    for name, tab in R.end_to_end_tables().items():
        assert tab.shape == (360, 6) and tab.dtype == np.float32
        got[name] = R.reference(tab, R.GRID, rows[:240], rows[240:])
        assert got[name]["sap_discrete"] == E.sap_discrete_from_score_matrix(got[name]["score_matrix"])
    print({k: round(v["sap_discrete"], 4) for k, v in got.items()})
    assert got["ideal"]["sap_discrete"] >= 0.4 and got["rotated"]["sap_discrete"] <= 0.15 and got["collapsed"]["sap_discrete"] <= 0.05
    assert got["ideal"]["score_matrix"].argmax(axis=0).tolist() == [0, 1, 2, 3]          # latent k holds factor k


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
    monkeypatch.setattr(_saplib, "lib", no_library)
    mean = torch.zeros(6, 4)
    ok = dict(n_train=4, n_test=2)
    for sizes, kw, msg in (([3, 3], ok, "does not enumerate"), ([3, 2], dict(n_train=0, n_test=2), r"n_train must lie in \[1, %d\]" % _saplib.MAX_ROWS),
                           ([3, 2], dict(n_train=_saplib.MAX_ROWS + 1, n_test=2), r"n_train must lie in \[1, %d\]" % _saplib.MAX_ROWS),
                           ([3, 2], dict(n_train=4, n_test=0), "n_test must be at least 1"), ([3, 2], dict(n_train=4, n_test=3), "n_train \\+ n_test must be at most 6"),
                           ([3, 2], {}, "n_train \\+ n_test must be at most 6"), ([1] * 8 + [6], ok, "at most 8"), ([0, 2], ok, "positive sizes"),
                           ([3, 2], dict(ok, C=0.0), "C must be a positive finite number"), ([3, 2], dict(ok, C=float("inf")), "C must be a positive"),
                           ([3, 2], dict(ok, C=float("nan")), "C must be a positive"), ([3, 2], dict(ok, C="1"), "C must be a positive"),
                           ([3, 2], dict(ok, rows=[0, 1, 2, 3, 4, 6]), r"in \[0, 6\)"), ([3, 2], dict(ok, rows=[0, 1, 2]), "rows must hold n_train \\+ n_test = 6"),
                           ([3, 2], dict(ok, rows=[]), "rows must hold n_train")):
        with pytest.raises(ValueError, match=msg):
            E.sap_discrete_from_table(mean, sizes, **kw)
    with pytest.raises(ValueError, match="at most %d classes" % _saplib.MAX_CLASSES):
        E.sap_discrete_from_table(torch.zeros(514, 1), [257, 2], n_train=10, n_test=5)
    with pytest.raises(ValueError, match="table"):
        E.sap_discrete_from_table(torch.zeros(6), [3, 2], **ok)
    with pytest.raises((TypeError, ValueError)):
        E.sap_discrete_from_table(mean, [3, 2], seed="x", **ok)
    bad = mean.clone()
    bad[4, 1] = float("nan")
    with pytest.raises(ValueError, match="NaN or an infinity"):
        E.sap_discrete_from_table(bad, [3, 2], **ok)
    with pytest.raises(_lib.DvaeHipError, match="no CPU"):
        E.sap_discrete_from_table(mean, [3, 2], **ok)
    model = _Model().train()
    ev = E.Evaluator(model, None, is_progress_bar=False)
    with pytest.raises(ValueError, match="known true factors"):
        ev.compute_sap_discrete(_Loader([0, 1, 2], None))
    for kw, msg in ((dict(n_train=0), "n_train must lie"), (dict(n_train=5, n_test=2), "n_train \\+ n_test must be at most 6"), (dict(ok, C=-1.0), "C must be")):
        with pytest.raises(ValueError, match=msg):
            ev.compute_sap_discrete(_Loader(_Factors(6), None), **kw)
    with pytest.raises(ValueError, match=r"data set of 5 images does not enumerate lat_sizes=\[3, 2\]"):
        ev.compute_sap_discrete(_Loader(_Factors(5), None), **ok)
    assert model.modes == [] and model.training
    loader = _Loader(_Factors(6), [(torch.rand(4, 1), None), (torch.rand(2, 1), None)])
    with pytest.raises(_lib.DvaeHipError, match="no CPU"):                 # valid arguments: the table is on the CPU
        ev.compute_sap_discrete(loader, **ok)
    assert model.modes == [False, False] and model.training               # encoded in eval mode, and the mode is as it was


def test_call_writes_the_sap_score_on_request(monkeypatch, tmp_path):
    seen = []
    model = _Model().train()
    ev = E.Evaluator(model, None, is_progress_bar=False, save_dir=str(tmp_path))
    result = {"sap_discrete": 0.25, "score_matrix": np.ones((2, 2)), "score_matrix_train": np.ones((2, 2)), "coef": np.zeros((2, 4, 2)),
              "n_iterations_max": 5, "n_train": 4, "n_test": 2, "C": 0.01}
    monkeypatch.setattr(ev, "compute_sap_discrete", lambda loader, **kw: seen.append((loader, kw, model.training)) or result)
    monkeypatch.setattr(ev, "compute_losses", lambda loader: {"loss": 1.5})
    loader = object()
    assert ev(loader) == (None, {"loss": 1.5}) and seen == [] and os.listdir(tmp_path) == ["test_losses.log"]
    assert ev(loader, is_losses=False, is_sap_discrete=True) == (None, None)
    assert seen == [(loader, {}, False)] and model.training
    assert ev(loader, is_losses=False, is_sap_discrete=True, sap_discrete_args=dict(n_train=4, n_test=2, C=1.0)) == (None, None)
    assert seen[-1] == (loader, dict(n_train=4, n_test=2, C=1.0), False)
    assert E.SAP_DISCRETE_FILE == "sap_discrete.log"
    assert json.load(open(tmp_path / "sap_discrete.log")) == {"sap_discrete": 0.25, "n_iterations_max": 5, "n_train": 4, "n_test": 2,
                                                              "C": 0.01}      # without the matrices and the coefficients
