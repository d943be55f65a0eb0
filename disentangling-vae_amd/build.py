"""Build libdvae_hip.so, libdvae_eval_hip.so, libdvae_score_hip.so, libdvae_info_hip.so, libdvae_irs_hip.so and libdvae_unsup_hip.so (gfx950) in-tree: hipcc cross-compiles without a GPU.

    python disentangling-vae_amd/build.py [--force] [--debug]

The libraries land in disentangling-vae_amd/lib/ (git-ignored build products).  Objects are rebuilt only
when a source / header is newer or the flags changed.
--debug (or DVAE_BUILD_DEBUG=1) adds -DDVAE_DEBUG_SWITCHES: the A/B / timing-ablation environment
switches and the experimental kernel variants they select (tools/README.md); the default (shipped)
library has none of them.  libdvae_eval_hip.so (include/dvae_eval_hip.h: the evaluation-side kernels,
csrc/elbo_decomp.hip) is a second target with the same flags and the same up-to-date logic under its own stamp;
libdvae_score_hip.so (include/dvae_score_hip.h: the FactorVAE / beta-VAE score kernels, csrc/factor_scores.hip) a third;
libdvae_info_hip.so (include/dvae_info_hip.h: the moments / joint-histogram kernels of the MIG, modularity and SAP scores,
csrc/factor_info.hip) a fourth;
libdvae_irs_hip.so (include/dvae_irs_hip.h: the group-mean / segmented-selection kernels of the interventional robustness score,
csrc/factor_irs.hip) a fifth;
libdvae_unsup_hip.so (include/dvae_unsup_hip.h: the covariance / pair-histogram kernels of the label-free scores,
csrc/latent_pairs.hip) a sixth.
"""
import glob
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(HERE, "build")
LIB = os.path.join(HERE, "lib", "libdvae_hip.so")
HEADERS = sorted(glob.glob(os.path.join(SRC, "*.h"))) + [os.path.join(HERE, "..", "include", "dvae_hip.h")]
SOURCES = ["conv_generic", "conv_mfma", "conv_down_dma", "conv_up_ws", "conv_wgrad_ws", "conv_thin", "conv_thin_ws", "conv_up_thin_mm", "linear", "linear_narrow", "gemm_dma", "linear_grouped", "fc_chain", "stage", "loss", "latent_wide",
           "metrics", "adam", "comm", "viz", "loglik", "plan", "capi"]
DEBUG_SOURCES = []          # experimental kernel files: only in --debug builds
# the evaluation-side library: its own sources, header and stamp; nothing of it is linked into libdvae_hip.so
EVAL_LIB = os.path.join(HERE, "lib", "libdvae_eval_hip.so")
EVAL_SOURCES = ["elbo_decomp"]
EVAL_HEADERS = HEADERS + [os.path.join(HERE, "..", "include", "dvae_eval_hip.h")]
# the disentanglement-score library: a third target of the same kind
SCORE_LIB = os.path.join(HERE, "lib", "libdvae_score_hip.so")
SCORE_SOURCES = ["factor_scores"]
SCORE_HEADERS = HEADERS + [os.path.join(HERE, "..", "include", "dvae_score_hip.h")]
# the information-score library (discretised MIG, modularity, SAP): a fourth
INFO_LIB = os.path.join(HERE, "lib", "libdvae_info_hip.so")
INFO_SOURCES = ["factor_info"]
INFO_HEADERS = HEADERS + [os.path.join(HERE, "..", "include", "dvae_info_hip.h")]
# the interventional-robustness-score library: a fifth
IRS_LIB = os.path.join(HERE, "lib", "libdvae_irs_hip.so")
IRS_SOURCES = ["factor_irs"]
IRS_HEADERS = HEADERS + [os.path.join(HERE, "..", "include", "dvae_irs_hip.h")]
# the label-free score library (Gaussian total correlation, Wasserstein correlation, latent-latent mutual information): a sixth
UNSUP_LIB = os.path.join(HERE, "lib", "libdvae_unsup_hip.so")
UNSUP_SOURCES = ["latent_pairs"]
UNSUP_HEADERS = HEADERS + [os.path.join(HERE, "..", "include", "dvae_unsup_hip.h")]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function"]


def _newer(a, b):
    return (not os.path.exists(b)) or os.path.getmtime(a) > os.path.getmtime(b)


def _build_target(hipcc, lib, sources, headers, flags, stamp, force, verbose):
    """Compile `sources` (objects rebuilt only when a source / header is newer or the stamped flags changed) and link `lib`."""
    want = " ".join(flags + sources)
    if not os.path.exists(stamp) or open(stamp).read() != want:
        force = True
    jobs = []
    for s in sources:
        src, obj = os.path.join(SRC, s + ".hip"), os.path.join(OBJ, s + ".o")
        if force or _newer(src, obj) or any(_newer(h, obj) for h in headers):
            jobs.append([hipcc] + flags + ["-c", src, "-o", obj])

    def run(cmd):
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed: %s\n%s" % (" ".join(cmd), r.stderr))
        return r.stderr

    with ThreadPoolExecutor(max_workers=8) as ex:
        for err in ex.map(run, jobs):
            if verbose and err.strip():
                sys.stderr.write(err)
    objs = [os.path.join(OBJ, s + ".o") for s in sources]
    if force or jobs or not os.path.exists(lib):
        run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + objs + ["-ldl"])
    with open(stamp, "w") as f:
        f.write(want)
    return lib


def build(force=False, verbose=True, debug=None):
    """Build the six libraries; returns the path of libdvae_hip.so."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if debug is None:
        debug = os.environ.get("DVAE_BUILD_DEBUG", "0") == "1"
    os.makedirs(OBJ, exist_ok=True)
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    flags = FLAGS + (["-DDVAE_DEBUG_SWITCHES"] if debug else [])
    sources = SOURCES + (DEBUG_SOURCES if debug else [])
    _build_target(hipcc, LIB, sources, HEADERS, flags, os.path.join(OBJ, "flags.txt"), force, verbose)
    _build_target(hipcc, EVAL_LIB, EVAL_SOURCES, EVAL_HEADERS, flags, os.path.join(OBJ, "flags_eval.txt"), force, verbose)
    _build_target(hipcc, SCORE_LIB, SCORE_SOURCES, SCORE_HEADERS, flags, os.path.join(OBJ, "flags_score.txt"), force, verbose)
    _build_target(hipcc, INFO_LIB, INFO_SOURCES, INFO_HEADERS, flags, os.path.join(OBJ, "flags_info.txt"), force, verbose)
    _build_target(hipcc, IRS_LIB, IRS_SOURCES, IRS_HEADERS, flags, os.path.join(OBJ, "flags_irs.txt"), force, verbose)
    _build_target(hipcc, UNSUP_LIB, UNSUP_SOURCES, UNSUP_HEADERS, flags, os.path.join(OBJ, "flags_unsup.txt"), force, verbose)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, debug=True if "--debug" in sys.argv else None))
