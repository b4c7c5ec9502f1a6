"""Golden data of the training-mode routing tail, from the reference itself (CPU; needs a checkout of the reference, imported through
oracle.refimport; the tests read only the .npz files this writes).

Runs the reference's DualGrainEncoder / TripleGrainEncoder in train mode with a tiny trunk (ch 32, z_channels 64, group-32,
2layer-fc-SiLu, B = 2), captures the router's inputs with a forward pre-hook and the noise F.gumbel_softmax draws (the RNG state
is saved around a wrapper that redraws the same noise), and takes the loss sum(h_out * R) + budget(gate) with the reference's
BudgetConstraint_* of the stage-1 config.  Stores inputs, router state_dict, noise, R, outputs, d budget / d gate and the
gradients of the router inputs and of every router parameter as tests/golden/route_train_{dual,triple}.npz
(tests/test_route_train.py::test_reference_golden).  Seeds are stepped until no cell's perturbed top-2 margin is below 1e-3, so
the test can demand identical decisions.

    python tools/gen_golden_route_train.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refimport  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
NORM, GATE = "group-32", "2layer-fc-SiLu"


def _encoder(nb):
    refimport.setup()
    if nb == 2:
        from modules.dynamic_modules.EncoderDual import DualGrainEncoder as Enc
        router = "modules.dynamic_modules.RouterDual.DualGrainFeatureRouter"
        mult = [1, 1, 2]
    else:
        from modules.dynamic_modules.EncoderTriple import TripleGrainEncoder as Enc
        router = "modules.dynamic_modules.RouterTriple.TripleGrainFeatureRouter"
        mult = [1, 1, 2, 2]
    cfg = {"target": router, "params": {"num_channels": 64, "normalization_type": NORM, "gate_type": GATE}}
    return Enc(ch=32, ch_mult=mult, num_res_blocks=1, attn_resolutions=[], in_channels=3, resolution=16, z_channels=64,
               router_config=cfg)


def _budget(nb):
    refimport.setup()
    from modules.dynamic_modules import budget
    if nb == 2:      # dqvae-dual-r-05: target 0.5, gamma 10, grain sizes scaled to the tiny trunk's 4 / 8 grids
        return budget.BudgetConstraint_RatioMSE_DualGrain(target_ratio=0.5, gamma=10.0, min_grain_size=4, max_grain_size=8)
    return budget.BudgetConstraint_NormedSeperateRatioMSE_TripleGrain(target_fine_ratio=0.3, target_median_ratio=0.3, gamma=1.0,
                                                                      min_grain_size=2, median_grain_size=4, max_grain_size=8)


def run(nb, seed):
    torch.manual_seed(seed)
    enc = _encoder(nb).train()
    with torch.no_grad():
        for n, p in enc.router.named_parameters():
            if "feature_norm" in n:
                p.add_(0.2 * torch.randn_like(p))
    cap = {}

    def pre_hook(_mod, args, kwargs):
        for k in ("h_coarse", "h_median", "h_fine"):
            if k in kwargs:
                kwargs[k].retain_grad()
                cap[k] = kwargs[k]
        return None

    enc.router.register_forward_pre_hook(pre_hook, with_kwargs=True)
    orig = F.gumbel_softmax

    def wrapped(logits, *a, **kw):
        st = torch.get_rng_state()
        cap["gumbels"] = -torch.empty_like(logits, memory_format=torch.legacy_contiguous_format).exponential_().log()
        cap["logits"] = logits.detach().clone()
        torch.set_rng_state(st)
        return orig(logits, *a, **kw)

    x = torch.randn(2, 3, 16, 16)
    F.gumbel_softmax = wrapped
    try:
        out = enc(x, None)
    finally:
        F.gumbel_softmax = orig
    z = cap["logits"] + cap["gumbels"]
    top = z.topk(2, dim=-1).values
    margin = float((top[..., 0] - top[..., 1]).min())
    if margin < 1e-3:
        return None
    key = "h_dual" if nb == 2 else "h_triple"
    h = out[key]
    R = torch.randn(h.shape, generator=torch.Generator().manual_seed(seed + 1))
    bud = _budget(nb)(out["gate"])
    g_gate = torch.autograd.grad(bud, out["gate"], retain_graph=True)[0]
    loss = (h * R).sum() + bud
    loss.backward()
    names = ["h_coarse", "h_median", "h_fine"] if nb == 3 else ["h_coarse", "h_fine"]
    rec = {"normalization_type": np.array(NORM), "gate_type": np.array(GATE), "seed": np.array(seed), "margin": np.array(margin),
           "gumbels": cap["gumbels"].numpy(), "R": R.numpy(), "h_out": h.detach().numpy(),
           "indices": out["indices"].numpy(), "codebook_mask": out["codebook_mask"].detach().numpy(),
           "gate": out["gate"].detach().numpy(), "g_gate_budget": g_gate.numpy()}
    for n in names:
        rec[n] = cap[n].detach().numpy()
        rec["grad." + n] = cap[n].grad.numpy()
    for n, v in enc.router.state_dict().items():
        rec["sd." + n] = v.numpy()
    for n, p in enc.router.named_parameters():
        rec["grad." + n] = p.grad.numpy()
    return rec


def main():
    for nb, tag in ((2, "dual"), (3, "triple")):
        for seed in range(100):
            rec = run(nb, seed)
            if rec is not None:
                break
        else:
            raise SystemExit("no seed with perturbed margins >= 1e-3")
        path = os.path.join(OUT, "route_train_%s.npz" % tag)
        np.savez_compressed(path, **rec)
        print("%s: seed %d, min perturbed margin %.3g, %d bytes" % (path, seed, rec["margin"], os.path.getsize(path)))


if __name__ == "__main__":
    main()
