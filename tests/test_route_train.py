"""GPU (-m gpu): the training-mode routing tail as one op (route_train_dual / route_train_triple, dvq_route_train_*_f32).
  * against the reference's own training step (tests/golden/route_train_*.npz, tools/gen_golden_route_train.py): its
    encoder's router inputs, gumbel noise and loss sum(h_out * R) + budget(gate);
  * against this package's torch-op router + the reference tail as torch ops at real shapes (B = 30, C = 256), every
    gate_type x normalization_type, the dual encoder with update_router=False;
  * seeded noise (gumbels=None draws what F.gumbel_softmax draws), bitwise determinism, the entropy router, errors.
Bar: indices and codebook_mask identical, gate exactly 0 off the hard index and within 2 ulp on it (the logits in no-gumbel
mode: 1e-5 relative), h_out 1e-6 relative, every gradient within 1e-4 * max |ref|."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dynamicvectorquantization_amd import _lib
from dynamicvectorquantization_amd.router import (DualGrainFeatureRouter, DualGrainFixedEntropyRouter,
                                                  TripleGrainFeatureRouter, route_select_dual_entropy, route_train_dual,
                                                  route_train_triple)
from tests._route_train_ref import branches as _branches
from tests._route_train_ref import check_gate as _check_gate
from tests._route_train_ref import check_h as _check_h
from tests._route_train_ref import make_router as _make_router
from tests._route_train_ref import margin as _margin
from tests._route_train_ref import nudge as _nudge
from tests._route_train_ref import torch_tail as _torch_tail

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _close_grad(a, b, what):
    ref = b.detach().double()
    tol = 1e-4 * float(ref.abs().max()) + 1e-30
    err = float((a.detach().double() - ref).abs().max())
    assert err <= tol, "%s: max err %g > %g" % (what, err, tol)


def _run_pair(nb, norm, gate_type, B=30, C=256, hc=None, update_router=True, seed=0):
    dev = torch.device("cuda:0")
    hc = hc or (16 if nb == 2 else 8)
    router = _make_router(nb, C, norm, gate_type, dev, 100 + seed)
    hs = _branches(nb, B, C, hc, hc, dev, 200 + seed)
    g = torch.Generator(device="cpu").manual_seed(300 + seed)
    S = 2 if nb == 2 else 4
    R = torch.randn((B, C, S * hc, S * hc), generator=g).to(dev)
    Q = torch.randn((B, nb, hc, hc), generator=g).to(dev)
    with torch.no_grad():
        logits = router(*(hs[::-1] if nb == 2 else [hs[2], hs[1], hs[0]]))
    gumbels = None
    if update_router:
        gumbels = _nudge(logits, -torch.empty_like(logits).exponential_(generator=None).log())
    else:
        assert float(_margin(logits).min()) > 1e-5, "pick another seed: a logit margin at fp32 noise"
    # torch-op side
    ref = _torch_tail(router, hs, gumbels, nb, update_router)
    loss = (ref["h"] * R).sum() + (ref["gate"] * Q).sum()
    params = [p for p in router.parameters()]
    gref = torch.autograd.grad(loss, hs + params)
    # the op
    if nb == 2:
        out = route_train_dual(router, hs[1], hs[0], gumbels=gumbels, update_router=update_router)
        h = out["h_dual"]
    else:
        out = route_train_triple(router, hs[2], hs[1], hs[0], gumbels=gumbels)
        h = out["h_triple"]
    loss2 = (h * R).sum() + (out["gate"] * Q).sum()
    gops = torch.autograd.grad(loss2, hs + params)
    assert torch.equal(out["indices"], ref["indices"]), "indices"
    assert torch.equal(out["codebook_mask"], ref["codebook_mask"]), "codebook_mask"
    _check_gate(out["gate"].detach(), ref["gate"].detach(), update_router)
    _check_h(h.detach(), ref["h"].detach())
    names = ["h%d" % i for i in range(nb)] + [n for n, _ in router.named_parameters()]
    for a, b, n in zip(gops, gref, names):
        _close_grad(a, b, n)


@pytest.mark.parametrize("norm", ["none", "group-32"])
@pytest.mark.parametrize("gate_type", ["1layer-fc", "2layer-fc-SiLu"])
def test_dual_vs_torch_ops(dev, norm, gate_type):
    _run_pair(2, norm, gate_type)


def test_dual_no_update_router_vs_torch_ops(dev):
    _run_pair(2, "group-32", "2layer-fc-SiLu", update_router=False)


@pytest.mark.parametrize("norm", ["none", "group-32"])
@pytest.mark.parametrize("gate_type", ["1layer-fc", "2layer-fc-SiLu", "2layer-fc-ReLu"])
def test_triple_vs_torch_ops(dev, norm, gate_type):
    _run_pair(3, norm, gate_type)


@pytest.mark.parametrize("nb", [2, 3])
def test_seeded_noise_matches_gumbel_softmax(dev, nb):
    """gumbels=None: the op draws F.gumbel_softmax's noise; under one seed it takes the torch path's decisions (a seed whose
    perturbed margins are all above 1e-4 is picked on the torch side)"""
    B, C, hc = 4, 64, 8
    router = _make_router(nb, C, "group-32", "2layer-fc-SiLu", dev, 7)
    hs = _branches(nb, B, C, hc, hc, dev, 8)
    args = hs[::-1] if nb == 2 else [hs[2], hs[1], hs[0]]
    with torch.no_grad():
        logits = router(*args)
        for s in range(200):
            torch.manual_seed(s)
            y = F.gumbel_softmax(logits, tau=1, dim=-1, hard=True)
            torch.manual_seed(s)
            gum = -torch.empty_like(logits).exponential_().log()
            if float(_margin(logits + gum).min()) > 1e-4:
                break
        else:
            pytest.fail("no seed with clear margins")
    torch.manual_seed(s)
    out = route_train_dual(router, hs[1], hs[0]) if nb == 2 else route_train_triple(router, hs[2], hs[1], hs[0])
    assert torch.equal(out["indices"], y.argmax(-1)), "decisions differ from F.gumbel_softmax under the same seed"
    assert torch.equal(out["gate"].detach() != 0, y.permute(0, 3, 1, 2) != 0)


@pytest.mark.parametrize("nb", [2, 3])
def test_bitwise_deterministic(dev, nb):
    B, C, hc = 30, 256, 16 if nb == 2 else 8
    router = _make_router(nb, C, "group-32", "2layer-fc-SiLu", dev, 11)
    hs = _branches(nb, B, C, hc, hc, dev, 12)
    gum = -torch.empty((B, hc, hc, nb), device=dev).exponential_().log()
    S = 2 if nb == 2 else 4
    R = torch.randn((B, C, S * hc, S * hc), device=dev)
    Q = torch.randn((B, nb, hc, hc), device=dev)
    res = []
    for _ in range(2):
        out = (route_train_dual(router, hs[1], hs[0], gumbels=gum) if nb == 2
               else route_train_triple(router, hs[2], hs[1], hs[0], gumbels=gum))
        h = out["h_dual" if nb == 2 else "h_triple"]
        grads = torch.autograd.grad((h * R).sum() + (out["gate"] * Q).sum(), hs + list(router.parameters()))
        res.append([h.detach(), out["gate"].detach(), out["indices"], out["codebook_mask"]] + list(grads))
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_entropy_router_delegates(dev, golden_dir):
    router = DualGrainFixedEntropyRouter(os.path.join(golden_dir, "entropy_thresholds_imagenet_train_patch-16.json"), 0.5)
    B, C, hc = 3, 64, 8
    hs = _branches(2, B, C, hc, hc, dev, 21)
    ent = torch.rand((B, hc, hc), device=dev) * 4.0
    R = torch.randn((B, C, 2 * hc, 2 * hc), device=dev)
    out = route_train_dual(router, hs[1], hs[0], entropy=ent, update_router=False)
    g1 = torch.autograd.grad((out["h_dual"] * R).sum(), hs)
    ref = route_select_dual_entropy(ent, router.fine_grain_threshold, hs[0], hs[1])
    g2 = torch.autograd.grad((ref["h_dual"] * R).sum(), hs)
    for k in ("h_dual", "indices", "codebook_mask", "gate"):
        assert torch.equal(out[k], ref[k]), k
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)


def test_errors(dev):
    router = DualGrainFeatureRouter(64, "group-32", "2layer-fc-SiLu")
    hs = [torch.randn(1, 64, 4, 4), torch.randn(1, 64, 8, 8)]
    with pytest.raises(_lib.DvqError):
        route_train_dual(router, hs[1], hs[0])                           # CPU tensors
    r12 = DualGrainFeatureRouter(12, "none", "1layer-fc").to(dev)
    with pytest.raises(_lib.DvqError):                                 # C % 8 != 0
        route_train_dual(r12, torch.randn(1, 12, 8, 8, device=dev), torch.randn(1, 12, 4, 4, device=dev))
    r700 = DualGrainFeatureRouter(704, "none", "1layer-fc").to(dev)
    with pytest.raises(_lib.DvqError):                                 # num_branches * C > 1280
        route_train_dual(r700, torch.randn(1, 704, 4, 4, device=dev), torch.randn(1, 704, 2, 2, device=dev))


@pytest.mark.parametrize("nb", [2, 3])
def test_reference_golden(dev, nb):
    """the reference encoder's training step (tools/gen_golden_route_train.py): router inputs, noise, R and the budget loss's
    gradient with respect to the gate as recorded; outputs and every gradient"""
    z = np.load(os.path.join(GOLDEN, "route_train_%s.npz" % ("dual" if nb == 2 else "triple")))
    t = lambda k: torch.from_numpy(z[k]).to(dev)
    C = z["h_coarse"].shape[1]
    cls = DualGrainFeatureRouter if nb == 2 else TripleGrainFeatureRouter
    router = cls(C, normalization_type=str(z["normalization_type"]), gate_type=str(z["gate_type"])).to(dev)
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd.")}
    router.load_state_dict(sd)
    names = ["h_coarse", "h_median", "h_fine"] if nb == 3 else ["h_coarse", "h_fine"]
    hs = [t(n).requires_grad_(True) for n in names]
    if nb == 2:
        out = route_train_dual(router, hs[1], hs[0], gumbels=t("gumbels"))
        h = out["h_dual"]
    else:
        out = route_train_triple(router, hs[2], hs[1], hs[0], gumbels=t("gumbels"))
        h = out["h_triple"]
    assert np.array_equal(out["indices"].cpu().numpy(), z["indices"])
    assert np.array_equal(out["codebook_mask"].cpu().numpy(), z["codebook_mask"])
    _check_gate(out["gate"].detach(), t("gate"), True)
    _check_h(h.detach(), t("h_out"))
    # the loss: sum(h_out * R) + budget(gate); the budget term enters through its recorded gradient d budget / d gate
    loss = (h * t("R")).sum() + (out["gate"] * t("g_gate_budget")).sum()
    pn = [n for n, _ in router.named_parameters()]
    grads = torch.autograd.grad(loss, hs + list(router.parameters()))
    for n, g in zip(names + pn, grads):
        _close_grad(g, t("grad." + n), n)
