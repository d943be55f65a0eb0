"""Cost of the InfoVAE / MMD-VAE regulariser (libdvae_mmd_hip.so, csrc/mmd_pairs.hip) and of the training step that carries it.

(a) The two launches alone (dvae_mmd_pairs + dvae_mmd_finish: value, dmu and dlv) at B = 64, 256, 1024, 2048 with D = 10 and
    B = 1024 with D = 32, both kernels, next to torch autograd -- forward + backward of tests/mmd_ref.py's regulariser_torch -- on
    the same GPU.  The gradients of both are compared before timing.
(b) The whole infovae training step against the VAE step of the same build, (3, 64, 64) at B = 1024 and (1, 32, 32) at B = 64, the
    shipped replay setting: what the regulariser adds to a step, to be held against (a).

Device events around each call; the candidates are INTERLEAVED (one repeat of each in turn, `--reps` rounds after a warm-up), so a
drift of the clocks lands on all of them; the median and the spread [min, max] are reported.  Inputs from a seed.  Prints one JSON
line per measurement and writes them to --out.

    python tools/mmd_time.py [--reps 30] [--out profiles/mmd_time.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "disentangling-vae_amd"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import mmd_ref  # noqa: E402
from dip_time import HP, interleaved_ms  # noqa: E402
from disvae_amd import _mmdlib  # noqa: E402
from disvae_amd.engine import _stream  # noqa: E402
from disvae_amd.models.losses import get_loss_f  # noqa: E402
from disvae_amd.models.vae import init_specific_model  # noqa: E402

W = 999.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mmd_time.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is nothing to time without it"
    lines = []

    def emit(what, t, **more):
        lines.append(json.dumps(dict({"what": what, "reps": args.reps, "median_ms": t[0], "spread_ms": t[1]}, **more)))
        print(lines[-1], flush=True)

    gen = torch.Generator(device="cuda").manual_seed(1)
    st = _stream()
    # ---- (a) the two launches alone
    for B, D in ((64, 10), (256, 10), (1024, 10), (2048, 10), (1024, 32)):
        z = torch.randn(B, D, generator=gen, device="cuda")
        p = torch.randn(B, D, generator=gen, device="cuda")
        mu = z - 0.3 * torch.randn(B, D, generator=gen, device="cuda")
        ws = torch.empty(_mmdlib.ws_doubles(B, D), dtype=torch.float64, device="cuda")
        out = torch.empty(_mmdlib.OUT_DOUBLES, dtype=torch.float64, device="cuda")
        dmu, dlv = torch.empty_like(z), torch.empty_like(z)
        h = mmd_ref.default_bandwidth(D)
        for kind in ("imq", "rbf"):
            def native(kind=kind):
                _mmdlib.call("dvae_mmd_pairs", z.data_ptr(), p.data_ptr(), B, D, _mmdlib.KERNELS[kind], h, 1, ws.data_ptr(), st)
                _mmdlib.call("dvae_mmd_finish", z.data_ptr(), mu.data_ptr(), B, D, W, ws.data_ptr(), dmu.data_ptr(), dlv.data_ptr(),
                             out.data_ptr(), None, st)
            tz = z.clone().requires_grad_(True)

            def autograd(kind=kind, tz=tz):
                return torch.autograd.grad(W * mmd_ref.regulariser_torch(tz, p, kind, h), [tz])
            native()
            (gz,) = autograd()
            err = float((gz - dmu).abs().max() / gz.abs().max())
            assert err < 1e-4, err
            t = interleaved_ms({"native": native, "torch": autograd}, args.reps, inner=20)
            emit("dvae_mmd_pairs + dvae_mmd_finish (value, dmu, dlv)", t["native"], B=B, D=D, kernel=kind, grad_vs_torch_rel=err)
            emit("torch autograd, forward + backward of the same regulariser", t["torch"], B=B, D=D, kernel=kind)
    # ---- (b) the whole step
    for img, B in (((3, 64, 64), 1024), ((1, 32, 32), 64)):
        steps = {}
        for loss, more in (("VAE", {}), ("infovae", dict(mmd_kernel="imq")), ("infovae rbf", dict(mmd_kernel="rbf"))):
            torch.manual_seed(3)
            model = init_specific_model("Burgess", img, 10).to("cuda")
            model.train()
            opt = torch.optim.Adam(model.parameters(), lr=5e-4)
            loss_f = get_loss_f(loss.split()[0], device=torch.device("cuda"), **dict(HP, **more))
            data = torch.rand((B,) + img, generator=gen, device="cuda")
            steps[loss] = (lambda loss_f=loss_f, model=model, opt=opt, data=data: loss_f.fused_step(data, model, opt, None))
        for fn in steps.values():                                     # past the warm-up of every replay mode
            for _ in range(6):
                fn()
        t = interleaved_ms(steps, args.reps, inner=10)
        for loss in steps:
            emit("whole training step, shipped replay setting", t[loss], loss=loss, img=list(img), B=B,
                 extra_vs_VAE_ms=round(t[loss][0] - t["VAE"][0], 5))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
