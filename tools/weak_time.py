"""Cost of the adaptive group posterior of Ada-GVAE / Ada-ML-VAE (libdvae_weak_hip.so, csrc/weak_pairs.hip) and of the training
step that carries it.

(a) The two launches alone (dvae_weak_aggregate_fwd with delta + dvae_weak_aggregate_bwd) at 64, 256, 1024, 2048 rows with D = 10
    and 1024 rows with D = 32, both aggregations, next to the same operator in torch on the same GPU -- forward + autograd backward of
    tests/weak_ref.py's aggregate_torch, the mask computed in torch as well.  Masks and gradients of both are compared before timing.
(b) The whole adagvae training step against the VAE step of the same build at the same row count, (1, 64, 64) with 256 rows and
    (3, 64, 64) with 1024 rows, the shipped replay setting: the per-layer FC path (about a dozen launches instead of two), the 4x4
    conv ends as launches of their own and the two new launches.

Device events around each call; the candidates are INTERLEAVED (one repeat of each in turn, `--reps` rounds after a warm-up), so a
drift of the clocks lands on all of them; the median and the spread [min, max] are reported.  Inputs from a seed.  Prints one JSON
line per measurement and writes them to --out.

    python tools/weak_time.py [--reps 30] [--out profiles/weak_time.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "disentangling-vae_amd"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import weak_ref  # noqa: E402
from dip_time import HP, interleaved_ms  # noqa: E402
from disvae_amd import _weaklib  # noqa: E402
from disvae_amd.engine import _stream  # noqa: E402
from disvae_amd.models.losses import get_loss_f  # noqa: E402
from disvae_amd.models.vae import init_specific_model  # noqa: E402


def torch_mask(mu, lv):
    P = mu.shape[0] // 2
    ma, mb, la, lb = mu[:P], mu[P:], lv[:P], lv[P:]
    delta = torch.exp(la - lb) + (mb - ma) ** 2 * torch.exp(-lb) - 1.0 + (lb - la)
    tau = 0.5 * delta.max(dim=1, keepdim=True).values + 0.5 * delta.min(dim=1, keepdim=True).values
    return delta < tau


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weak_time.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is nothing to time without it"
    lines = []

    def emit(what, t, **more):
        lines.append(json.dumps(dict({"what": what, "reps": args.reps, "median_ms": t[0], "spread_ms": t[1]}, **more)))
        print(lines[-1], flush=True)

    gen = torch.Generator(device="cuda").manual_seed(1)
    st = _stream()
    # ---- (a) the two launches alone
    for rows, D in ((64, 10), (256, 10), (1024, 10), (2048, 10), (1024, 32)):
        P = rows // 2
        mu = torch.randn(rows, D, generator=gen, device="cuda")
        lv = -6.0 * torch.rand(rows, D, generator=gen, device="cuda")
        ml = torch.stack((mu, lv), dim=-1).reshape(rows, 2 * D).contiguous()
        g = torch.randn(rows, 2 * D, generator=gen, device="cuda")
        ml_agg, dml = torch.empty_like(ml), torch.empty_like(ml)
        shared = torch.empty(P, dtype=torch.int64, device="cuda")
        delta = torch.empty(P, D, device="cuda")
        for kind in weak_ref.KINDS:
            def native(kind=kind):
                _weaklib.call("dvae_weak_aggregate_fwd", ml.data_ptr(), P, D, _weaklib.KINDS[kind], ml_agg.data_ptr(), shared.data_ptr(),
                              delta.data_ptr(), st)
                dml.copy_(g)                                              # the backward launch works in place
                _weaklib.call("dvae_weak_aggregate_bwd", ml.data_ptr(), shared.data_ptr(), P, D, _weaklib.KINDS[kind], dml.data_ptr(), st)
            tmu, tlv = mu.clone().requires_grad_(True), lv.clone().requires_grad_(True)

            def autograd(kind=kind, tmu=tmu, tlv=tlv):
                am, al = weak_ref.aggregate_torch(tmu, tlv, kind, torch_mask(tmu.detach(), tlv.detach()))
                return torch.autograd.grad((am * g[:, 0::2]).sum() + (al * g[:, 1::2]).sum(), [tmu, tlv])
            native()
            autograd()
            # the comparison: torch at the DEVICE's mask (an entry at rounding distance of tau may be masked either way)
            sh = ((shared.unsqueeze(1) >> torch.arange(D, device="cuda")) & 1).bool()
            flips = int((sh != torch_mask(mu, lv)).sum())
            am, al = weak_ref.aggregate_torch(tmu, tlv, kind, sh)
            gmu, glv = torch.autograd.grad((am * g[:, 0::2]).sum() + (al * g[:, 1::2]).sum(), [tmu, tlv])
            err = float(max((gmu - dml[:, 0::2]).abs().max() / gmu.abs().max(), (glv - dml[:, 1::2]).abs().max() / glv.abs().max()))
            assert err < 1e-4 and flips <= 2, (err, flips)
            t = interleaved_ms({"native": native, "torch": autograd}, args.reps, inner=20)
            emit("dvae_weak_aggregate_fwd (with delta) + copy of the gradient + dvae_weak_aggregate_bwd", t["native"], rows=rows, D=D,
                 aggregation=kind, grad_vs_torch_rel=err)
            emit("torch, forward + autograd backward of the same operator", t["torch"], rows=rows, D=D, aggregation=kind)
    # ---- (b) the whole step
    for img, rows in (((1, 64, 64), 256), ((3, 64, 64), 1024)):
        steps = {}
        for loss in ("VAE", "adagvae", "adamlvae"):
            torch.manual_seed(3)
            model = init_specific_model("Burgess", img, 10).to("cuda")
            model.train()
            opt = torch.optim.Adam(model.parameters(), lr=5e-4)
            loss_f = get_loss_f(loss, device=torch.device("cuda"), **HP)
            data = torch.rand((rows,) + img, generator=gen, device="cuda")
            steps[loss] = (lambda loss_f=loss_f, model=model, opt=opt, data=data: loss_f.fused_step(data, model, opt, None))
        for fn in steps.values():                                     # past the warm-up of every replay mode
            for _ in range(6):
                fn()
        t = interleaved_ms(steps, args.reps, inner=10)
        for loss in steps:
            emit("whole training step, shipped replay setting", t[loss], loss=loss, img=list(img), rows=rows,
                 extra_vs_VAE_ms=round(t[loss][0] - t["VAE"][0], 5))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
