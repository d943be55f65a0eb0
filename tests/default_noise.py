"""The noise one training iteration draws for itself, restated for the tests (not collected).

The contract ("The noise contract"): per iteration, in this order,

  device generator   FactorVAE: a discarded [B, D] draw (the reference's full-batch model(data) before FactorKLoss raises
                     ValueError, training.py:153, quirk Q4), [B // 2, D] for model(data1) (losses.py:254), [B // 2, D] for
                     sample_latent(data2) (losses.py:286);
                     every other loss: one [B, D] draw (torch.randn_like, vae.py:67);
  CPU generator      FactorVAE: D times torch.randperm(B // 2) (losses.py:505); every other loss: nothing.

``predraw`` makes exactly these draws with plain torch.randn / torch.randperm from seeded global generators, so that a step
fed with them (the injected-noise step every parity test pins to the oracle) can be compared bit for bit with a step that
draws for itself after the same seeding.  On the CPU (tests/test_default_noise_host.py) both streams share the one CPU
generator: discarded draw, eps, eps2, then the permutations -- the order of oracle.disvae_oracle.OracleTrainer.
"""
import torch


def device_draws(loss, B, D):
    """Shapes taken from the DEVICE generator by one training iteration, in order."""
    if loss == "factor":
        return [(B, D), (B // 2, D), (B // 2, D)]
    return [(B, D)]


def cpu_draws(loss, B, D):
    """Arguments of the torch.randperm calls one training iteration makes on the CPU generator, in order."""
    if loss == "factor":
        return [B // 2] * D
    return []


def seed(dev_seed, cpu_seed, device):
    """Seed the global generators the step draws from.  torch.manual_seed seeds every device generator as well, so it goes
    first; on the CPU there is only the one generator."""
    torch.manual_seed(cpu_seed)
    if torch.device(device).type == "cuda":
        torch.cuda.manual_seed(dev_seed)


def rng_states(device):
    """(device generator state or None on the CPU, CPU generator state)."""
    on_gpu = torch.device(device).type == "cuda"
    return (torch.cuda.get_rng_state() if on_gpu else None), torch.get_rng_state()


def predraw(loss, sizes, D, dev_seed, cpu_seed, device):
    """The draws of len(sizes) iterations with batch sizes `sizes` -> (noise, device generator state, CPU generator state).

    noise[i] is {"eps": [B, D]} or, for FactorVAE, {"eps1": [Bh, D], "eps2": [Bh, D], "perms": int64 [D, Bh] (CPU)}; the
    discarded draw is made and dropped.  Build the models BEFORE calling this (their initialisation consumes the CPU
    generator) and take test data from a private torch.Generator."""
    seed(dev_seed, cpu_seed, device)
    noise = []
    for B in sizes:
        drawn = [torch.randn(shape, device=device) for shape in device_draws(loss, B, D)]
        perms = [torch.randperm(n) for n in cpu_draws(loss, B, D)]
        if loss == "factor":
            noise.append({"eps1": drawn[1], "eps2": drawn[2], "perms": torch.stack(perms)})
        else:
            noise.append({"eps": drawn[0]})
    dev_state, cpu_state = rng_states(device)
    return noise, dev_state, cpu_state
