"""CPU: the plumbing the score libraries share -- csrc/table_stats.h and csrc/last_error.h stay the one home of their helpers,
disvae_amd/_cabi.py is the one loader behind the eight bindings, build.py's TARGETS drives every build and tools/isa_identity.py,
and evaluate.py's mutual information from counts is the expression the two *_from_statistics functions used to spell out."""
import importlib.util
import os
import re

import numpy as np
import pytest

from disvae_amd import _cabi, _dcilib, _diplib, _evallib, _infolib, _irslib, _lib, _scorelib, _udrlib, _unsuplib
from disvae_amd.evaluate import mutual_information_from_counts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "disentangling-vae_amd", "csrc")
DUMMY = 1 << 20                                                   # aligned non-NULL address, never dereferenced
# module -> (its source, its *_last_error symbol, an entry point, arguments that pass every check, a required pointer among them)
BINDINGS = {
    _evallib: ("elbo_decomp.hip", "dvae_eval_last_error", "dvae_eval_joint_logq",
               [DUMMY, DUMMY, DUMMY, 5, 3, 4, DUMMY, DUMMY, DUMMY, None], 0),
    _scorelib: ("factor_scores.hip", "dvae_score_last_error", "dvae_score_group_var",
                [DUMMY, DUMMY, 50, 3, 4, 5, DUMMY, DUMMY, DUMMY, None], 8),
    _infolib: ("factor_info.hip", "dvae_info_last_error", "dvae_info_joint_hist",
               [DUMMY, DUMMY, DUMMY, DUMMY, 60, 3, 3, 10, 20, 12, None, DUMMY, None], 3),
    _irslib: ("factor_irs.hip", "dvae_irs_last_error", "dvae_irs_group_means",
              [DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, 60, 3, 3, 10, 12, 13, 5, DUMMY, DUMMY, DUMMY, None], 13),
    _unsuplib: ("latent_pairs.hip", "dvae_unsup_last_error", "dvae_unsup_moments",
                [DUMMY, DUMMY, 60, 3, 10, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, None], 9),
    _udrlib: ("latent_ranks.hip", "dvae_udr_last_error", "dvae_udr_ranks",
              [DUMMY, DUMMY, 60, 3, 10, DUMMY, DUMMY, None], 6),
    _dcilib: ("boosted_trees.hip", "dvae_dci_last_error", "dvae_dci_predict",
              [DUMMY, DUMMY, 60, 3, 10, 3, 5, 0.1, DUMMY, DUMMY, DUMMY, None], 10),
    _diplib: ("dip_cov.hip", "dvae_dip_last_error", "dvae_dip_moments",
              [DUMMY, DUMMY, 40, 3, DUMMY, DUMMY], 4),
}


def _load(name, *path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- 1. one home ----------------------------------------------------------------------------------------------------------------
def test_score_helpers_have_one_home():
    """csrc/table_stats.h is the one definition of the helpers the score kernels share and csrc/last_error.h of a library's error
    text: no per-file copy grows back, and every library has exactly one translation unit that owns its error text."""
    text = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h"))}

    def homes(pattern):
        return [f for f, t in text.items() if re.search(pattern, t, re.M)]
    for name in ("put_f64", "get_f64", "chunks_of", "lesser"):            # a definition: a return type, the name, a body
        assert homes(r"^[ \w]*\b(?:void|double|int|T)\s+%s\s*\([^;{]*\)\s*\{" % name) == ["table_stats.h"], name
    # the count of edges <= x stays in its two kernels: every shared form of it changed their machine code (table_stats.h says so)
    assert homes(r"\bbelow\s*\+=.*<=\s*x\b") == ["factor_info.hip", "latent_pairs.hip"] and "edges <= x" in text["table_stats.h"]
    assert homes(r"^void set_error\([^;{]*\)\s*\{") == ["last_error.h"]
    assert homes(r"\bthread_local\b") == ["last_error.h"]
    build = _load("dvae_build_plumbing", "disentangling-vae_amd", "build.py")
    assert len(build.TARGETS) == 9
    for _name, sources, _header in build.TARGETS:
        includes = [len(re.findall(r'^#include "last_error\.h"', text[s + ".hip"], re.M)) for s in sources]
        assert sum(includes) == 1 and max(includes) == 1, (sources, includes)
    assert not [f for f in homes(r'#include "last_error\.h"') if f.endswith(".h")]


# ---- 2. the binding -------------------------------------------------------------------------------------------------------------
def test_binding_fails_loudly_without_the_library_or_a_symbol(tmp_path):
    missing = str(tmp_path / "libdvae_eval_hip.so")
    b = _cabi.Binding(missing, _evallib.SIGNATURES, _evallib._RESTYPE, "dvae_eval_last_error", "evaluation")
    with pytest.raises(_lib.DvaeHipError) as e:
        b.lib()
    assert missing in str(e.value) and "build.py" in str(e.value)
    assert str(e.value) == ("libdvae_eval_hip.so not found at %s -- build it with `python disentangling-vae_amd/build.py` "
                            "(there is no CPU / PyTorch fallback for the evaluation kernels)" % missing)
    table = dict(_evallib.SIGNATURES, dvae_eval_no_such_entry_point=[])
    b = _cabi.Binding(_evallib.LIB_PATH, table, _evallib._RESTYPE, "dvae_eval_last_error", "evaluation")
    with pytest.raises(AttributeError, match="dvae_eval_no_such_entry_point"):
        b.lib()
    with pytest.raises(AttributeError, match="dvae_eval_no_such_entry_point"):       # ... and a failed load is not kept as loaded
        b.lib()


@pytest.mark.parametrize("mod", list(BINDINGS), ids=lambda m: m.__name__.rsplit(".", 1)[-1])
def test_call_raises_with_the_librarys_own_error_text(mod):
    source, last_error, name, good, required = BINDINGS[mod]
    assert last_error in mod.SIGNATURES and mod._RESTYPE[last_error] is not None
    h = mod.lib()
    assert h is mod.lib()                                                 # loaded once
    args = good[:required] + [None] + good[required + 1:]
    with pytest.raises(_lib.DvaeHipError) as e:
        mod.call(name, *args)
    own = getattr(h, last_error)().decode()
    assert "invalid argument" in own and source in own                    # the library's own text: its source reported it
    assert str(e.value) == "%s failed (-1): %s" % (name, own)
    for other, (_src, other_error, *_rest) in BINDINGS.items():           # every library keeps its own buffer
        if other is not mod:
            assert source not in getattr(other.lib(), other_error)().decode()


@pytest.mark.parametrize("mod", list(BINDINGS), ids=lambda m: m.__name__.rsplit(".", 1)[-1])
def test_call_loads_through_the_modules_lib(mod, monkeypatch):
    class Boom(Exception):
        pass

    def boom():
        raise Boom("lib() of the module was asked")
    monkeypatch.setattr(mod, "lib", boom)
    _source, _last_error, name, good, _required = BINDINGS[mod]
    with pytest.raises(Boom, match="was asked"):
        mod.call(name, *good)


# ---- 3. the build table ---------------------------------------------------------------------------------------------------------
def test_build_table_drives_the_exported_names_and_the_identity_tool():
    build = _load("dvae_build_plumbing", "disentangling-vae_amd", "build.py")
    assert [name for name, _s, _h in build.TARGETS] == ["", "eval", "score", "info", "irs", "unsup", "udr", "dci", "dip"]
    for name, sources, header in build.TARGETS:
        prefix = name.upper() + "_" if name else ""
        lib, srcs, headers = (getattr(build, prefix + suffix) for suffix in ("LIB", "SOURCES", "HEADERS"))
        assert srcs == sources and all(os.path.exists(os.path.join(build.SRC, s + ".hip")) for s in srcs)
        assert os.path.basename(lib) == ("libdvae_%s_hip.so" % name if name else "libdvae_hip.so")
        assert os.path.dirname(os.path.abspath(lib)) == os.path.join(ROOT, "disentangling-vae_amd", "lib")
        assert header == ("dvae_%s_hip.h" % name if name else "dvae_hip.h")
        assert sorted(os.path.basename(h) for h in headers if "include" in h.split(os.sep)) == sorted({"dvae_hip.h", header})
        assert all(os.path.exists(h) for h in headers)
        csrc_headers = {os.path.basename(h) for h in headers} - {"dvae_hip.h", header}
        assert csrc_headers == {f for f in os.listdir(CSRC) if f.endswith(".h")}          # every csrc header rebuilds every target
        assert build._target(name, sources, header)[3] == os.path.join(build.OBJ, "flags_%s.txt" % name if name else "flags.txt")
    for i, (_n, a, _h) in enumerate(build.TARGETS):
        for _m, b, _g in build.TARGETS[i + 1:]:
            assert not set(a) & set(b), (a, b)
    union = [s for _n, sources, _h in build.TARGETS for s in sources]
    assert len(union) == len(set(union))
    isa = _load("dvae_isa_identity_plumbing", "tools", "isa_identity.py")
    assert sorted(isa.ALL_SOURCES) == sorted(union) and len(isa.ALL_SOURCES) == len(union) == 31
    assert build.ALL_SOURCES == union


# ---- 4. mutual information from counts ------------------------------------------------------------------------------------------
def _mi_as_it_was_spelled_out(block):
    """The block that information_scores_from_statistics and unsupervised_scores_from_statistics each held."""
    S = block[0].sum()
    row, col = block.sum(axis=2, keepdims=True), block.sum(axis=1, keepdims=True)
    nz = block > 0
    term = np.zeros_like(block)
    term[nz] = block[nz] / S * np.log((block * S)[nz] / (row * col)[nz])
    return term.sum(axis=(1, 2))


MI_TABLES = {
    "2x2": [[3, 1], [2, 6]],
    "3x5": [[4, 0, 7, 1, 2], [1, 9, 3, 0, 5], [6, 2, 2, 8, 1]],
    "zero row": [[5, 2, 3], [0, 0, 0], [1, 7, 4]],
    "one cell": [[0, 0], [0, 11]],
    "independent": [[2, 4, 6], [3, 6, 9]],                               # outer product of (2, 3) and (1, 2, 3)
}


@pytest.mark.parametrize("key", list(MI_TABLES))
def test_mutual_information_from_counts_is_the_expression_it_replaced(key):
    table = np.asarray(MI_TABLES[key], dtype=np.int64)
    block = np.stack([table, table[::-1].copy()]).astype(np.float64)     # two tables over the same rows, as the callers pass
    got, want = mutual_information_from_counts(block), _mi_as_it_was_spelled_out(block)
    assert got.dtype == np.float64 and got.shape == (2,)
    assert got.tobytes() == want.tobytes()                                # bit for bit
    assert (got >= 0).all()
    if key in ("independent", "one cell"):
        assert got[0] == 0.0                                              # c S / (row col) = 1 exactly: log 1 = 0
    else:
        assert got[0] > 0.0
