"""CPU: the host side of the DCI scores -- the eighth library's C-ABI (include/dvae_dci_hip.h == disvae_amd/_dcilib.py == the built
libdvae_dci_hip.so), its row of build.py's TARGETS, the LDS budget, dci_from_importance on hand-made matrices, the fp64
restatement (tests/dci_ref.py) against the installed scikit-learn, the preconditions the GPU tests rely on, and the argument errors
raised before any library load.

The restatement against scikit-learn 1.7.2's GradientBoostingClassifier(n_estimators, random_state = 0 .. 7).  sklearn is not unique:
among splits of equal gain it keeps the first in a feature order drawn from random_state.  Measured on the CPU, per case the
largest per-entry width of the hull (max - min over the 8 seeds) of importances / train accuracy / the two scores, and the
restatement's largest distance outside the hull widened by 25 % (never by less than 1e-12):

    S = 96,  D = 4, C = 3,  5 stages    width 2.0e-02 / 1.0e-02 / 2.1e-02    distance 0
    S = 300, D = 6, C = 5, 10 stages    width 9.6e-04 / 0       / 1.2e-03    distance 0
    two classes, S = 96, D = 4, 5       width 3.2e-16 / 0       / 3.3e-16    distance 0 (the floor of 1e-12 governs)

The tie-break among features is not all that differs.  The residuals of the first stages take two values, so DIFFERENT splits of a
small node -- the mirror image (2 | 38 rows on one feature, 38 | 2 on another), or two features that isolate the same rows -- have
the same gain in exact arithmetic; which wins is decided by the last bit of sum_left and sum_total, in sklearn (whose order of
summation follows its sample permutation) as in the restatement (which adds in row order).  Eight seeds sample that noise eight
times and the restatement is a ninth draw: on the seeded tables of this file it lies inside every hull, on another draw of the
S = 300 table (same recipe, another seed) it lay 2.4e-3 outside an importance hull of width 4.5e-3.  The bound stays as it was set;
the trees themselves are compared exactly on a table without such ties (test_first_stage_trees_are_sklearns).
"""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import dci_ref as R
import disvae_amd
from disvae_amd import _cabi, _dcilib, _lib, _udrlib
from disvae_amd import evaluate as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dvae_dci_hip.h")
CSRC = os.path.join(ROOT, "disentangling-vae_amd", "csrc")


def _build():
    spec = importlib.util.spec_from_file_location("dvae_build_dci", os.path.join(ROOT, "disentangling-vae_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- 1. the library -----------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _nm(path, *flags):
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin")
    assert nm, "no nm on this machine"
    return subprocess.run([nm] + list(flags) + [path], capture_output=True, text=True, check=True).stdout


def test_header_ctypes_table_and_exports_agree(monkeypatch):
    declared = sorted(set(re.findall(r"\b(dvae_dci_[a-zA-Z0-9_]+)\s*\(", _header())))
    assert declared == sorted(_dcilib.SIGNATURES) and len(declared) == 6
    assert declared == sorted(["dvae_dci_version", "dvae_dci_last_error", "dvae_dci_trees", "dvae_dci_fit_ws_floats",
                               "dvae_dci_fit", "dvae_dci_predict"])
    exported = sorted(set(re.findall(r" T (dvae_\w+)", _nm(os.path.abspath(_dcilib.LIB_PATH), "-D", "--defined-only"))))
    assert exported == declared
    kinds = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_long: "l", ctypes.c_double: "d"}
    for name, params in re.findall(r"\b(dvae_dci_[a-zA-Z0-9_]+)\s*\(([^)]*)\)", _header()):
        got = []
        for prm in [x.strip() for x in params.split(",") if x.strip() != "void"]:
            got.append("p" if "*" in prm else ("l" if prm.startswith("long") else ("d" if prm.startswith("double") else "i")))
        assert got == [kinds[t] for t in _dcilib.SIGNATURES[name]], name
    macros = {k: int(v) for k, v in re.findall(r"#define (DVAE_DCI_\w+) (\d+)", _header())}
    mirrored = {"DVAE_DCI_VERSION": _dcilib.VERSION, "DVAE_DCI_MAX_D": _dcilib.MAX_D, "DVAE_DCI_MAX_CLASSES": _dcilib.MAX_CLASSES,
                "DVAE_DCI_MAX_ROWS": _dcilib.MAX_ROWS, "DVAE_DCI_MAX_STAGES": _dcilib.MAX_STAGES, "DVAE_DCI_THREADS": _dcilib.THREADS,
                "DVAE_DCI_ROW_LDS_BYTES": _dcilib.ROW_LDS_BYTES, "DVAE_DCI_LDS_SCRATCH": _dcilib.LDS_SCRATCH,
                "DVAE_DCI_NODES": _dcilib.NODES, "DVAE_DCI_NODE_STATS": _dcilib.NODE_STATS,
                "DVAE_DCI_LAUNCHES_PER_STAGE": _dcilib.LAUNCHES_PER_STAGE}
    assert macros == mirrored                                            # every macro of the header, none besides
    assert (_dcilib.MAX_D, _dcilib.MAX_CLASSES) == (64, 256) and _dcilib.MAX_ROWS >= 10000
    assert _dcilib.lib().dvae_dci_version() == _dcilib.VERSION == 1
    assert os.path.basename(_dcilib.LIB_PATH) == "libdvae_dci_hip.so"
    binding = open(_dcilib.__file__).read()
    assert 'Binding.for_library("dci", SIGNATURES, _RESTYPE' in binding and "LIB_PATH = _binding.path" in binding
    assert _dcilib._binding.last_error == "dvae_dci_last_error" and _dcilib._binding.signatures is _dcilib.SIGNATURES
    monkeypatch.setenv("DVAE_DCI_HIP_LIB", "/elsewhere/lib.so")              # the override, read when a binding is made
    assert _cabi.Binding.for_library("dci", {}, {}, "").path == "/elsewhere/lib.so"
    for name in ("dci_from_table", "dci_from_importance"):
        assert name in disvae_amd.__all__ and getattr(disvae_amd, name) is getattr(E, name)
    assert [_dcilib.lib().dvae_dci_trees(C) for C in (0, 1, 2, 3, 256, 257)] == [0, 1, 1, 3, 256, 0]
    assert [_dcilib.trees(C) for C in (1, 2, 3, 256)] == [1, 1, 3, 256]


def test_lds_budget():
    """A workgroup of the split search holds one sorted column of the selected rows in LDS: residual fp64, value fp32, node byte
    per row, every thread the same number of rows, plus the scan's wave records -- within the 160 KB of a CDNA4 compute unit, and
    10 000 rows (disentanglement_lib's training set) fit."""
    assert _dcilib.ROW_LDS_BYTES == 8 + 4 + 1
    assert _dcilib.MAX_ROWS % _dcilib.THREADS == 0
    assert _dcilib.ROW_LDS_BYTES * _dcilib.MAX_ROWS + _dcilib.LDS_SCRATCH <= _dcilib.LDS_BYTES == 160 * 1024
    waves = _dcilib.THREADS // 64
    assert waves * 4 * (4 + 8 + 4 + 8 + 4 + 4) <= _dcilib.LDS_SCRATCH      # per wave and open node: the scan's and the best split's record
    assert 10000 <= _dcilib.MAX_ROWS
    src = open(os.path.join(CSRC, "boosted_trees.hip")).read()
    assert "DCI_LDS_MAX + DVAE_DCI_LDS_SCRATCH <= 160 * 1024" in src


def test_dci_row_is_a_row_of_the_build_table():
    """what test_build_table_drives_the_exported_names_and_the_identity_tool demands of every row of TARGETS, of the dci row -- and
    that "dci" is IN the table, not what the table is: the next library is one more row."""
    build = _build()
    rows = [row for row in build.TARGETS if row[0] == "dci"]
    assert [tuple(row) for row in rows] == [("dci", ["boosted_trees"], "dvae_dci_hip.h")]
    names = [n for n, _s, _h in build.TARGETS]
    assert len(names) == len(set(names))
    taken = {s for n, sources, _h in build.TARGETS if n != "dci" for s in sources}
    text = {f: open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))}
    for name, sources, header in rows:
        prefix = name.upper() + "_"
        lib, srcs, headers = (getattr(build, prefix + suffix) for suffix in ("LIB", "SOURCES", "HEADERS"))
        assert srcs == sources and all(os.path.exists(os.path.join(build.SRC, s + ".hip")) for s in srcs)
        assert os.path.basename(lib) == "libdvae_%s_hip.so" % name
        assert os.path.dirname(os.path.abspath(lib)) == os.path.join(ROOT, "disentangling-vae_amd", "lib")
        assert header == "dvae_%s_hip.h" % name
        assert sorted(os.path.basename(h) for h in headers if "include" in h.split(os.sep)) == sorted({"dvae_hip.h", header})
        assert all(os.path.exists(h) for h in headers)
        assert {os.path.basename(h) for h in headers} - {"dvae_hip.h", header} == {f for f in os.listdir(CSRC) if f.endswith(".h")}
        assert build._target(name, sources, header)[3] == os.path.join(build.OBJ, "flags_%s.txt" % name)
        assert not set(sources) & taken                                   # no source is shared with another row
        taken |= set(sources)
        includes = [len(re.findall(r'^#include "last_error\.h"', text[s + ".hip"], re.M)) for s in sources]
        assert sum(includes) == 1 and max(includes) == 1
        assert os.path.exists(lib)                                        # build() built it
    assert set(build.DCI_SOURCES) <= set(build.ALL_SOURCES)               # tools/isa_identity.py compares them


def test_source_obeys_the_rules_of_the_shared_plumbing():
    src = open(os.path.join(CSRC, "boosted_trees.hip")).read()
    assert not re.search(r"\bthread_local\b", src) and not re.search(r"^void set_error\(", src, re.M)
    for name in ("put_f64", "get_f64", "chunks_of", "lesser"):
        assert not re.search(r"^[ \w]*\b(?:void|double|int|T)\s+%s\s*\([^;{]*\)\s*\{" % name, src, re.M), name
    assert not re.search(r"\bbelow\s*\+=.*<=\s*x\b", src)
    assert "table_stats.h" not in src                                   # none of its helpers is needed here: no dead include
    assert not re.search(r"atomic\w*\s*\(\s*\(?\s*(float|double)", src) and "while" not in src      # no float atomics, no spinning
    assert "hipDeviceSynchronize" not in src and "hipStreamSynchronize" not in src and "hipMemcpy" not in src   # calls only enqueue
    assert "cooperative" not in src.lower()


def test_call_raises_with_the_librarys_own_error_text():
    h = _dcilib.lib()
    assert h is _dcilib.lib()
    dummy = 1 << 20                                               # aligned non-NULL address, never dereferenced
    #      table  rows   order  labels N    D  S   C  stages lr  init raw    prior  ws     imp    nsplit feat   stats  stream
    fit = [dummy, dummy, dummy, dummy, 200, 4, 96, 3, 5, 0.1, 1, dummy, dummy, dummy, dummy, dummy, dummy, dummy, None]
    #          table  rows   N    D  S   C  stages lr  feat   stats  raw    stream
    predict = [dummy, dummy, 200, 4, 96, 3, 5, 0.1, dummy, dummy, dummy, None]

    def put(good, i, v):
        return good[:i] + [v] + good[i + 1:]
    bad = [("dvae_dci_fit", put(fit, i, None)) for i in (0, 2, 3, 11, 12, 13, 14, 15, 16, 17)]
    bad += [("dvae_dci_predict", put(predict, i, None)) for i in (0, 8, 9, 10)]
    for i in (4, 5, 6, 7, 8):                                           # N, D, S, C, n_stages: zero and negative
        bad += [("dvae_dci_fit", put(fit, i, 0)), ("dvae_dci_fit", put(fit, i, -1))]
    for i in (2, 3, 4, 5, 6):
        bad += [("dvae_dci_predict", put(predict, i, 0)), ("dvae_dci_predict", put(predict, i, -1))]
    bad += [("dvae_dci_fit", put(fit, 5, _dcilib.MAX_D + 1)), ("dvae_dci_fit", put(fit, 6, _dcilib.MAX_ROWS + 1)),
            ("dvae_dci_fit", put(fit, 7, _dcilib.MAX_CLASSES + 1)), ("dvae_dci_fit", put(fit, 8, _dcilib.MAX_STAGES + 1)),
            ("dvae_dci_fit", put(put(fit, 1, None), 4, _dcilib.MAX_ROWS + 1)),              # all rows of a larger table
            ("dvae_dci_fit", put(fit, 9, 0.0)), ("dvae_dci_fit", put(fit, 9, float("nan"))), ("dvae_dci_fit", put(fit, 9, 1.5)),
            ("dvae_dci_fit", put(fit, 10, 2)), ("dvae_dci_fit", put(fit, 13, dummy + 4)),    # ws aligned to 4 bytes only
            ("dvae_dci_predict", put(predict, 3, _dcilib.MAX_D + 1)), ("dvae_dci_predict", put(predict, 5, _dcilib.MAX_CLASSES + 1)),
            ("dvae_dci_predict", put(predict, 7, -0.1))]
    for name, args in bad:
        with pytest.raises(_lib.DvaeHipError) as e:
            _dcilib.call(name, *args)
        own = h.dvae_dci_last_error().decode()
        assert "invalid argument" in own and "boosted_trees.hip" in own, (name, args, own)
        assert str(e.value) == "%s failed (-1): %s" % (name, own)
    assert "boosted_trees.hip" not in _udrlib.lib().dvae_udr_last_error().decode()          # every library keeps its own buffer
    assert h.dvae_dci_fit_ws_floats(200, 4, _dcilib.MAX_ROWS + 1, 3, 5) == 0 and h.dvae_dci_fit_ws_floats(200, 65, 96, 3, 5) == 0
    assert h.dvae_dci_fit_ws_floats(200, 4, 96, 257, 5) == 0 and h.dvae_dci_fit_ws_floats(200, 4, 96, 3, 0) == 0
    assert h.dvae_dci_fit_ws_floats(200, 4, 0, 3, 5) == h.dvae_dci_fit_ws_floats(200, 4, 200, 3, 5) >= 1
    S, D, T, n = 96, 4, 3, 5                         # residuals, node statistics, gains, importances; (lo, hi); flags; node bytes
    assert h.dvae_dci_fit_ws_floats(200, D, S, 3, n) == 2 * (T * S + T * 15 * 5 + T * 4 * D + n * T * D) + T * 4 * D * 2 + n * T + (T * S + 3) // 4


# ---- 2. dci_from_importance on hand-made matrices ---------------------------------------------------------------------------------
@pytest.mark.parametrize("scores", [R.dci_scores, E.dci_from_importance], ids=["reference", "evaluate"])
def test_scores_of_known_matrices(scores):
    for D, K in ((3, 3), (5, 5)):
        d, c = scores(np.eye(D))
        assert abs(d - 1) <= 1e-8 and abs(c - 1) <= 1e-8                  # the + 1e-11 of disentanglement_lib keeps it off 1
        d, c = scores(np.eye(D)[np.random.default_rng(D).permutation(D)] * 0.3)
        assert abs(d - 1) <= 1e-8 and abs(c - 1) <= 1e-8
    for shape in ((4, 3), (3, 5)):
        d, c = scores(np.full(shape, 0.25))
        assert abs(d) <= 1e-12 and abs(c) <= 1e-12
        d, c = scores(np.zeros(shape))                                    # the fall-back: every latent and factor weighs alike
        assert abs(d) <= 1e-12 and abs(c) <= 1e-12
    M = np.array([[1.0, 0.0], [0.0, 1.0], [0.0, 0.0]])                    # a dead latent takes nothing from either score
    d, c = scores(M)
    assert abs(d - 1) <= 1e-8 and abs(c - 1) <= 1e-8
    M = np.array([[0.5, 0.5], [0.0, 0.0]])                                # one latent carries both factors
    d, c = scores(M)
    assert abs(d) <= 1e-8 and abs(c - 1) <= 1e-8
    rng = np.random.default_rng(0)
    for _ in range(3):
        M = rng.random((6, 4))
        assert np.allclose(E.dci_from_importance(M), R.dci_scores(M), rtol=0, atol=1e-14)


def test_scores_are_scipys_entropies():
    from scipy import stats                                              # disentanglement_lib's own entropies: no skip without it
    M = np.random.default_rng(1).random((5, 3)) ** 3
    per_code = 1.0 - stats.entropy(M.T + 1e-11, base=M.shape[1])
    per_factor = 1.0 - stats.entropy(M + 1e-11, base=M.shape[0])
    want = (float((per_code * M.sum(axis=1) / M.sum()).sum()), float((per_factor * M.sum(axis=0) / M.sum()).sum()))
    assert np.allclose(E.dci_from_importance(M), want, rtol=0, atol=1e-14)


# ---- 3. the restatement against the installed scikit-learn ------------------------------------------------------------------------
def _heap(tree):
    """sklearn's depth-first node table -> the heap order of the dump: (feature [15], threshold [15], n [15], value [15])"""
    f, thr, n, value = np.full(15, -1), np.zeros(15), np.zeros(15), np.zeros(15)

    def walk(i, h):
        n[h], value[h] = tree.n_node_samples[i], tree.value[i, 0, 0]
        if tree.children_left[i] >= 0:
            f[h], thr[h] = tree.feature[i], tree.threshold[i]
            walk(tree.children_left[i], 2 * h + 1)
            walk(tree.children_right[i], 2 * h + 2)
    walk(0, 0)
    return f, thr, n, value


def test_first_stage_trees_are_sklearns():
    """On a table where no two features induce the same partition of a node (one strongly informative continuous column, S = 96;
    the gap report says so before it is relied on) the first-stage trees ARE sklearn's: feature, threshold bits and node counts
    exactly, values within 1e-12 relative.  Nodes that are pure but for rounding -- sklearn goes on splitting some of them, by
    rounding noise in its subtracted sums -- are compared down to where the restatement stops."""
    from sklearn import ensemble                                         # the one yardstick of the restatement: no skip without it
    X, labels, C, n_stages = R.case("clean")
    assert (X.shape, C, n_stages) == ((96, 4), 3, 1)
    ours = R.fit(X, labels, C, 1, gaps=True)
    assert min(ours["gaps"]) >= 1e-3, ours["gaps"]                        # no two partitions near each other
    model = ensemble.GradientBoostingClassifier(n_estimators=1, random_state=0).fit(X, labels)
    assert np.abs(model._raw_predict_init(X) - np.tile(R.prior(labels, C), (96, 1))).max() <= 1e-15
    compared = 0
    for k in range(C):
        f, thr, n, value = _heap(model.estimators_[0, k].tree_)
        for h in range(15):
            if ours["stats"][0, k, h, 2] == 0:
                continue
            assert n[h] == ours["stats"][0, k, h, 2], (k, h)
            if ours["feature"][0, k, h] >= 0:
                assert f[h] == ours["feature"][0, k, h] and thr[h].tobytes() == ours["stats"][0, k, h, 0].tobytes(), (k, h)
                compared += 1
            elif f[h] < 0:                                                # a leaf in both: the Newton step
                assert abs(value[h] - ours["stats"][0, k, h, 1]) <= 1e-12 * abs(value[h]), (k, h)
            else:                                                         # sklearn split a node that is pure but for rounding
                own = ours["stats"][0, k, h]
                assert R.mse(own[2], own[3], own[4]) <= R.EPS
    assert compared >= 4
    assert np.abs(model._raw_predict(X) - ours["raw"]).max() <= 1e-12 * np.abs(ours["raw"]).max()


HULL_CASES = {"S96_D4_C3_5": "basic", "S300_D6_C5_10": "five_class", "two_class": "two_class"}


@pytest.mark.parametrize("key", list(HULL_CASES))
def test_restatement_within_the_hull_of_eight_sklearn_seeds(key):
    """The restatement's importance vector, train accuracy and the two scores (of the [D, 2] matrix of its importances beside a
    fixed second column) within the per-entry min-max hull of GradientBoostingClassifier(random_state = 0 .. 7), widened by 25 % of
    its width and never by less than 1e-12.  Tables: one informative column, one rounded to 1 / 2, one constant.  The measured
    widths and distances are in the module docstring (the test prints them)."""
    from sklearn import ensemble                                         # the one yardstick of the restatement: no skip without it
    X, labels, C, n_stages = R.case(HULL_CASES[key])
    ours = R.fit(X, labels, C, n_stages)
    second = np.linspace(1.0, 2.0, X.shape[1])                           # a fixed column beside the importances: a [D, 2] matrix

    def figures(importance, accuracy):
        d, c = R.dci_scores(np.stack([importance, second / second.sum()], axis=1))
        return np.concatenate([importance, [accuracy, d, c]])
    got = figures(R.normalised_importance(ours["importance"], ours["n_split"]), (R.classes_of(ours["raw"], C) == labels).mean())
    seeds = []
    for seed in range(8):
        model = ensemble.GradientBoostingClassifier(n_estimators=n_stages, random_state=seed).fit(X, labels)
        seeds.append(figures(model.feature_importances_, model.score(X, labels)))
    lo, hi = np.min(seeds, axis=0), np.max(seeds, axis=0)
    widen = np.maximum(0.25 * (hi - lo), 1e-12)
    outside = np.maximum(np.maximum(lo - widen - got, got - hi - widen), 0.0)
    print("%s: hull widths %s, distance outside the widened hull %s" % (key, np.array2string(hi - lo, precision=2),
                                                                       np.array2string(outside, precision=2)))
    print("largest width: importance %.2g, accuracy %.2g, scores %.2g" % ((hi - lo)[:-3].max(), (hi - lo)[-3], (hi - lo)[-2:].max()))
    assert (outside == 0).all(), (key, outside)


# ---- 4. the preconditions of the GPU tests, from the restatement alone -------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CASES))
def test_preconditions_of_the_gpu_cases(name):
    X, labels, C, n_stages = R.case(name)
    with_gaps = name in R.CAP_CASES
    ours = R.fit(X, labels, C, n_stages, gaps=with_gaps)
    out = R.verify(X, labels, C, ours["feature"], ours["stats"], ours["raw"])      # the verifier accepts the restatement's own dump
    assert out["other_choice"] == 0 and out["nodes"] >= n_stages
    assert n_stages <= 10 and len(X) <= _dcilib.MAX_ROWS
    if with_gaps:                                                        # the cap of the GPU test rests on this share
        gaps = np.array(ours["gaps"])
        assert len(gaps) == out["nodes"] and (gaps >= 1e-9).mean() >= 0.98, (name, (gaps >= 1e-9).mean())
    f, n = ours["feature"].reshape(-1, 15), ours["stats"].reshape(-1, 15, 5)[:, :, 2]
    if name == "pure":                                                   # a node turns pure at depth 1 and its sibling goes on
        assert any((f[i, a] < 0 and n[i, a] > 0 and f[i, b] >= 0) for i in range(len(f)) for a, b in ((1, 2), (2, 1)))
    if name in ("basic", "two_class"):
        assert (X[:, 2] == X[0, 2]).all() and len(np.unique(X[:, 1])) < 20 and (f != 2).all() and (f == 1).any()
    if name == "chunk_below":
        assert len(X) == _dcilib.THREADS and len(R.case("chunk_above")[0]) == _dcilib.THREADS + 1
    if name == "large_lds":
        rows_per_thread = -(-len(X) // _dcilib.THREADS)
        assert _dcilib.ROW_LDS_BYTES * rows_per_thread * _dcilib.THREADS > 64 * 1024
        assert _dcilib.ROW_LDS_BYTES * (rows_per_thread - 1) * _dcilib.THREADS <= 64 * 1024


def test_restatement_continues_and_predicts():
    X, labels, C, _n = R.case("basic")
    whole, first = R.fit(X, labels, C, 5), R.fit(X, labels, C, 2)
    second = R.fit(X, labels, C, 3, raw=first["raw"])
    assert second["raw"].tobytes() == whole["raw"].tobytes()
    assert np.concatenate([first["feature"], second["feature"]]).tobytes() == whole["feature"].tobytes()
    prior = np.tile(R.prior(labels, C), (len(X), 1))
    assert np.abs(R.predict(X, whole["feature"], whole["stats"], prior) - whole["raw"]).max() <= 1e-13


# ---- 5. argument errors, before any library load ------------------------------------------------------------------------------
def test_every_argument_check_raises_before_a_library_load(monkeypatch):
    def boom():
        raise AssertionError("a library was loaded")
    monkeypatch.setattr(_dcilib, "lib", boom)
    t = torch.zeros(60, 4)
    sizes = (3, 4, 5)
    small = dict(n_train=40, n_test=20)
    for mean, lat_sizes, kw, exc, text in [
            (torch.zeros(60), sizes, small, ValueError, r"\[N, D\] table"),
            (t, (), small, ValueError, "positive sizes"),
            (t, (3, 0, 5), small, ValueError, "positive sizes"),
            (torch.zeros(600, 4), (2, 300), small, ValueError, "at most 256 classes"),
            (t, sizes, dict(n_train=0, n_test=20), ValueError, "n_train"),
            (t, sizes, dict(n_train=_dcilib.MAX_ROWS + 1, n_test=20), ValueError, "n_train"),
            (t, sizes, dict(n_train=40, n_test=0), ValueError, "n_test"),
            (t, sizes, dict(n_train=41, n_test=20), ValueError, "without replacement"),
            (t, sizes, dict(n_stages=0, **small), ValueError, "n_stages"),
            (t, sizes, dict(n_stages=_dcilib.MAX_STAGES + 1, **small), ValueError, "n_stages"),
            (torch.zeros(60, 65), sizes, small, ValueError, "between 1 and 64"),
            (torch.zeros(59, 4), sizes, small, ValueError, "does not enumerate"),
            (t, sizes, dict(rows=list(range(59)), **small), ValueError, "n_train \\+ n_test"),
            (t, sizes, dict(rows=[60] * 60, **small), ValueError, "rows must hold"),
            (t * float("nan"), sizes, small, ValueError, "NaN or an infinity"),
            (t, sizes, small, _lib.DvaeHipError, "needs the table on the GPU")]:
        with pytest.raises(exc, match=text):
            E.dci_from_table(mean, lat_sizes, **kw)
    with pytest.raises(TypeError):
        E.dci_from_table(t, sizes, n_bins=20)
    for bad in (np.zeros(3), np.zeros((0, 3))):
        with pytest.raises(ValueError, match="non-empty"):
            E.dci_from_importance(bad)


class _Loader:
    def __init__(self, n, lat_sizes=None):
        self.dataset = list(range(n))
        if lat_sizes is not None:
            self.dataset = type("Factors", (list,), {"lat_sizes": np.array(lat_sizes), "lat_names": tuple("abc")})(range(n))

    def __iter__(self):
        raise AssertionError("the loader was walked")


def test_compute_dci_checks_before_it_encodes(monkeypatch):
    from disvae_amd.models.vae import init_specific_model
    monkeypatch.setattr(_dcilib, "lib", lambda: (_ for _ in ()).throw(AssertionError("a library was loaded")))
    model = init_specific_model("Burgess", (1, 32, 32), 3)
    ev = E.Evaluator(model, None, is_progress_bar=False)
    model.train()
    with pytest.raises(ValueError, match="known true factors"):
        ev.compute_dci(_Loader(60))
    for n, kw, exc in ((60, dict(n_train=50, n_test=20), ValueError), (60, dict(n_train=40, n_test=20, n_stages=0), ValueError),
                       (59, dict(n_train=30, n_test=20), ValueError), (60, dict(n_bins=3), TypeError)):
        with pytest.raises(exc):
            ev.compute_dci(_Loader(n, (3, 4, 5)), **kw)
    assert model.training
    with pytest.raises(ValueError):
        ev(_Loader(60, (3, 4, 5)), is_losses=False, is_dci=True)          # the defaults ask for 15 000 rows of 60
