"""The training-mode routing tail (csrc/router_train.hip, route_train_dual / route_train_triple) restated for its tests:

  * Router64: the feature routers' formula in float64 on the CPU, written out (GroupNorm(groups, C, eps=1e-6) or identity per
    branch, average pool onto the coarse grid, concat coarse -> fine, NHWC, Linear or Linear -> SiLU | ReLU -> Linear with any
    hidden width), built from the state dict of the module under test;
  * torch_tail: the reference's training tail (EncoderDual.py:131-156 / EncoderTriple.py:145-183) as torch ops with explicit
    noise and tau; it runs the fp32 torch-op chain and, on Router64 and float64 inputs, the float64 statement;
  * CASES: the ragged shapes, each row naming the edge of the kernels it is there for, and the predicates that say so;
  * the host arithmetic of router_train.hip (slab rule, split-K chunk, workspace layout, rt_dgg_kernel's nq, tile counts) in
    Python, written from the .hip text;
  * the per-slice error rule of tests/test_route_train_shapes.py and tools/route_train_accuracy.py.
Nothing here calls the code under test except kernel_graph / run_kernel."""
import copy
import functools
import math

import torch
import torch.nn as nn

from dynamicvectorquantization_amd.router import (DualGrainFeatureRouter, TripleGrainFeatureRouter, route_train_dual,
                                                  route_train_triple)

U = 2.0 ** -24                                       # one fp32 rounding
FLOOR_ROUNDINGS = 16                                 # floor of the slice rule: sixteen roundings of the slice's largest value
MARGIN = 1e-3                                        # top-2 margin of the perturbed float64 logits that every cell must have

# (nb, B, C, hc, wc, norm, gate_type, hidden or None, tau)
CASES = [
    # one cell: 3 idle waves in the head kernels; Wo = 2 so nq = 128 > C; B = 1; F = 16
    (2, 1, 8, 1, 1, "none", "1layer-fc", None, 1.0),
    # N = 105 (N % 4, N % 64, ncell % 32 all != 0); Wo = 14 (256 % Wo != 0); 1 channel per group
    (2, 3, 8, 5, 7, "group-8", "2layer-fc-SiLu", 16, 1.0),
    # F = 24 (k-tail of the GEMM's 16-step); Wo = 20; ReLU'; tau
    (3, 1, 8, 3, 5, "group-4", "2layer-fc-ReLu", 24, 0.5),
    # 3 channels per group; F = 48; hidden != F and < 64; the second M tile holds 2 rows (N = 66)
    (2, 2, 24, 3, 11, "group-8", "2layer-fc-SiLu", 40, 2.0),
    # pseudo-groups of the pool kernel (C / 8 = 5); F = 120; hidden 72 (the second N tile is 8 wide)
    (3, 2, 40, 2, 3, "none", "2layer-fc-SiLu", 72, 1.0),
    # Wo = 258 > 256: nq = 1 and the column loop of rt_dgg_kernel, dual
    (2, 1, 8, 1, 129, "group-2", "1layer-fc", None, 1.0),
    # Wo = 260 > 256, triple
    (3, 1, 8, 1, 65, "none", "1layer-fc", None, 0.7),
    # N = 513: two split-K slabs, the second partial
    (2, 1, 16, 19, 27, "group-16", "2layer-fc-SiLu", 32, 1.0),
    # N = 8320: the slab count capped at RT_NS_MAX = 16, kc rounded up to 528
    (2, 2, 8, 64, 65, "group-8", "2layer-fc-SiLu", 24, 1.0),
    # F = 216 (4 N tiles, the last 24 wide); 9 channels per group; the image-order sums over B = 5
    (3, 5, 72, 4, 4, "group-8", "2layer-fc-SiLu", 216, 1.0),
]
# the dual encoder with update_router=False (no noise, gate = the logits): 3 x 8 x 5 x 7
CASE_NO_UPDATE = (2, 3, 8, 5, 7, "group-4", "2layer-fc-SiLu", 16, 1.0)
ROW_ONE_CELL, ROW_105, ROW_F24, ROW_WO258, ROW_N513, ROW_N8320 = 0, 1, 2, 5, 7, 8
SEED_NO_UPDATE = 0                                   # a seed at which every float64 logit margin is >= MARGIN (asserted)


def case_id(row):
    nb, B, C, hc, wc, norm, gate_type, hidden, tau = row
    return "nb%d-B%d-C%d-%dx%d-%s-%s-h%s-tau%g" % (nb, B, C, hc, wc, norm, gate_type.split("-")[-1], hidden, tau)


def groups_of(norm):
    return 0 if norm == "none" else int(norm.split("-")[-1])


# ---- the host arithmetic of router_train.hip, restated ---------------------------------------------------------------------
RT_NS_MAX = 16


def rt_a256(x):
    return (x + 255) // 256 * 256


def rt_slabs(N):
    return max(1, min(RT_NS_MAX, (N + 511) // 512))


def rt_split(K, ns):
    """rt_gemm / rt_reduce: (kc, nz) -- the k range of one slab, rounded up to the GEMM's 16-step, and the slabs that exist"""
    kc = ((K + ns - 1) // ns + 15) // 16 * 16
    return kc, (K + kc - 1) // kc


def rt_layout_total(nb, B, C, hc, wc, groups, H):
    ncell = hc * wc
    N, F, G = B * ncell, nb * C, nb
    W2c = H if H > 0 else F
    ns = rt_slabs(N)
    sizes = [B * nb * (groups if groups > 0 else 1) * 8,      # stats
             B * F * ncell * 4,                                 # pool
             N * F * 4 if groups > 0 else 0,                    # xn
             N * F * 4,                                         # x
             N * H * 4, N * H * 4,                              # apre, hh
             N * G * 4, N * 4, N * 4,                           # y, kidx, gg
             N * 4, N * G * 4, N * H * 4, N * F * 4, N * F * 4,  # dgg, dl, da, dx, dxc
             B * F * 4, B * F * 4, B * F * 16,                  # p1, p2, coef
             ns * H * F * 4, ns * G * W2c * 4, ns * H * 4, ns * G * 4]   # sw1, sw2, sb1, sb2
    return sum(rt_a256(s) for s in sizes)


def rt_nq(Wo):
    """rt_dgg_kernel: channel lanes per output column"""
    return 256 // Wo if Wo <= 256 else 1


def geometry(row):
    """every quantity the kernels of router_train.hip branch or tile on, for one row"""
    nb, B, C, hc, wc, norm, gate_type, hidden, tau = row
    groups = groups_of(norm)
    S = 2 if nb == 2 else 4
    ncell, F = hc * wc, nb * C
    N = B * ncell
    H = 0 if gate_type == "1layer-fc" else (hidden if hidden is not None else F)
    ns = rt_slabs(N)
    kc, nz = rt_split(N, ns)
    return dict(nb=nb, B=B, C=C, hc=hc, wc=wc, groups=groups, S=S, ncell=ncell, F=F, N=N, H=H, tau=tau, Wo=S * wc,
                nq=rt_nq(S * wc), cpg=C // groups if groups > 0 else 8, ns=ns, kc=kc, nz=nz, last_slab=N - (nz - 1) * kc,
                m_tiles=(N + 63) // 64, n_tiles_F=(F + 63) // 64,
                act={"1layer-fc": 0, "2layer-fc-SiLu": 1, "2layer-fc-ReLu": 2}[gate_type])


# ---- float64 restatement of the router --------------------------------------------------------------------------------------
class Router64(nn.Module):
    """the feature routers' forward in float64, from the state dict of the module under test (`gate.*` or `gate.0.*` /
    `gate.2.*`, `feature_norm_{coarse,median,fine}.*`); groups and the activation are not in a state dict and are given"""

    def __init__(self, state_dict, nb, groups, act):
        super().__init__()
        self.nb, self.groups, self.act = nb, groups, act
        self.keys = list(state_dict)
        for k, v in state_dict.items():
            self.register_parameter(k.replace(".", "__"), nn.Parameter(v.detach().cpu().double().clone()))

    def p(self, key):
        return getattr(self, key.replace(".", "__"))

    def named(self):
        return [(k, self.p(k)) for k in self.keys]

    def _norm(self, x, name):
        if self.groups == 0:
            return x
        B, C, H, W = x.shape
        xg = x.reshape(B, self.groups, -1)
        mean = xg.mean(-1, keepdim=True)
        var = ((xg - mean) ** 2).mean(-1, keepdim=True)                  # biased
        xh = ((xg - mean) / torch.sqrt(var + 1e-6)).reshape(B, C, H, W)
        w, b = self.p("feature_norm_%s.weight" % name), self.p("feature_norm_%s.bias" % name)
        return xh * w[None, :, None, None] + b[None, :, None, None]

    @staticmethod
    def _pool(x, s):
        B, C, H, W = x.shape
        return x.reshape(B, C, H // s, s, W // s, s).mean((3, 5))

    def forward(self, h_fine, h_coarse, h_median=None, entropy=None):
        feats = [self._norm(h_coarse, "coarse")]
        if self.nb == 3:
            feats.append(self._pool(self._norm(h_median, "median"), 2))
        feats.append(self._pool(self._norm(h_fine, "fine"), 4 if self.nb == 3 else 2))
        x = torch.cat(feats, dim=1).permute(0, 2, 3, 1)
        if self.act == 0:
            return x @ self.p("gate.weight").t() + self.p("gate.bias")
        a = x @ self.p("gate.0.weight").t() + self.p("gate.0.bias")
        a = a * torch.sigmoid(a) if self.act == 1 else a.clamp(min=0.0)
        return a @ self.p("gate.2.weight").t() + self.p("gate.2.bias")


def torch_tail(router, branches, gumbels, nb, update_router=True, tau=1.0):
    """the reference's training tail (EncoderDual.py:131-156 / EncoderTriple.py:145-183) as torch ops, F.gumbel_softmax's
    arithmetic with explicit noise; in the dtype of its inputs"""
    if nb == 2:
        h_coarse, h_fine = branches
        gate = router(h_fine=h_fine, h_coarse=h_coarse)
    else:
        h_coarse, h_median, h_fine = branches
        gate = router(h_fine=h_fine, h_median=h_median, h_coarse=h_coarse)
    scaled = update_router
    if update_router:
        y_soft = ((gate + gumbels) / tau).softmax(-1)
        index = y_soft.max(-1, keepdim=True)[1]
        y_hard = torch.zeros_like(gate).scatter_(-1, index, 1.0)
        gate = y_hard - y_soft.detach() + y_soft
    gate = gate.permute(0, 3, 1, 2)
    indices = gate.argmax(dim=1)
    S = 2 if nb == 2 else 4
    rep = lambda t, s: t.repeat_interleave(s, dim=-1).repeat_interleave(s, dim=-2)
    ir = rep(indices, S).unsqueeze(1)
    if nb == 2:
        h = torch.where(ir == 0, rep(h_coarse, 2), h_fine)
        masks = (0.25, 1.0)
    else:
        hm = rep(h_median, 2)
        h = torch.where(ir == 0, rep(h_coarse, 4), hm)
        h = torch.where(ir == 1, hm, h)
        h = torch.where(ir == 2, h_fine, h)
        masks = (0.0625, 0.25, 1.0)
    if scaled:
        h = h * rep(gate.max(dim=1, keepdim=True)[0], S)
    cmask = torch.full_like(ir, masks[-1], dtype=torch.float32)
    for i, m in enumerate(masks[:-1]):
        cmask = torch.where(ir == i, torch.full_like(cmask, m), cmask)
    return {"h": h, "indices": indices, "codebook_mask": cmask, "gate": gate}


def branches(nb, B, C, hc, wc, dev, seed):
    """the branches coarse -> fine, a different scale and offset per branch"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    out = []
    for i in range(nb):
        s = (1 << i) if nb == 3 else 1 + i
        out.append((torch.randn((B, C, hc * s, wc * s), generator=g) * (0.5 + i) + 0.1 * i).to(dev).requires_grad_(True))
    return out


def make_router(nb, C, norm, gate_type, dev, seed, hidden=None):
    """the module under test with perturbed GroupNorm affines; hidden: another hidden width than nb * C (router.gate replaced by
    a Sequential of the same layout: route_train_* takes "a module with its attribute names")"""
    torch.manual_seed(seed)
    cls = DualGrainFeatureRouter if nb == 2 else TripleGrainFeatureRouter
    r = cls(C, normalization_type=norm, gate_type=gate_type)
    if hidden is not None and gate_type != "1layer-fc" and hidden != nb * C:
        act = nn.SiLU() if gate_type == "2layer-fc-SiLu" else nn.ReLU()
        r.gate = nn.Sequential(nn.Linear(nb * C, hidden), act, nn.Linear(hidden, nb))
    r = r.to(dev)
    with torch.no_grad():
        for n, p in r.named_parameters():
            if "feature_norm" in n:           # non-trivial GroupNorm affines
                p.add_(0.2 * torch.randn_like(p))
    return r


def margin(z):
    top = z.topk(2, dim=-1).values
    return top[..., 0] - top[..., 1]


def nudge(logits, gumbels, thr=MARGIN):
    """raise the winner's noise where the perturbed top-2 margin is below thr (decisions then identical at fp32 noise); the
    noise keeps its dtype, the margins are taken in that of the logits"""
    z = logits + gumbels.to(logits.dtype)
    small = margin(z) < thr
    bump = torch.zeros_like(gumbels).scatter_(-1, z.argmax(-1, keepdim=True), 2 * thr)
    g = torch.where(small.unsqueeze(-1), gumbels + bump, gumbels)
    assert float(margin(logits + g.to(logits.dtype)).min()) >= thr
    return g


def check_gate(gate, ref_gate, hard):
    if hard:
        off = ref_gate == 0
        assert torch.equal(gate == 0, off), "gate zero pattern"
        on = ~off
        a, b = gate[on], ref_gate[on]
        ulp = torch.abs(torch.nextafter(b, torch.full_like(b, 2.0)) - b)
        assert bool(((a - b).abs() <= 2 * ulp).all()), "gate on the hard index beyond 2 ulp"
    else:
        assert bool(((gate - ref_gate).abs() <= 1e-5 * ref_gate.abs().max()).all()), "logits"


def check_h(h, ref):
    assert bool(((h - ref).abs() <= 1e-6 * ref.abs() + 1e-30).all()), "h_out beyond 1e-6 relative"


# ---- one row: inputs, the float64 reference, the two fp32 evaluations ---------------------------------------------------------
BRANCH_NAMES = {2: ["h_coarse", "h_fine"], 3: ["h_coarse", "h_median", "h_fine"]}


class Inputs:
    """fp32 inputs of one row on the CPU: the module under test, the branches coarse -> fine, the (nudged) noise, the cotangents
    R of h_out and Q of the gate; `logits64` are Router64's"""

    def __init__(self, row, seed, update_router=True, tau=None):
        nb, B, C, hc, wc, norm, gate_type, hidden, row_tau = row
        self.row, self.nb, self.update_router = row, nb, update_router
        self.tau = row_tau if tau is None else tau
        self.geo = geometry(row)
        cpu = torch.device("cpu")
        self.router = make_router(nb, C, norm, gate_type, cpu, 100 + seed, hidden)
        self.hs = branches(nb, B, C, hc, wc, cpu, 200 + seed)
        g = torch.Generator(device="cpu").manual_seed(300 + seed)
        S = self.geo["S"]
        self.R = torch.randn((B, C, S * hc, S * wc), generator=g)
        self.Q = torch.randn((B, nb, hc, wc), generator=g)
        self.router64 = Router64(self.router.state_dict(), nb, self.geo["groups"], self.geo["act"])
        with torch.no_grad():
            self.logits64 = self._call(self.router64, [h.detach().double() for h in self.hs])
        self.nudged = 0
        if update_router:
            raw = -torch.empty((B, hc, wc, nb)).exponential_(generator=g).log()
            self.gumbels = nudge(self.logits64, raw)
            self.nudged = int((self.gumbels != raw).any(-1).sum())
        else:
            self.gumbels = None

    def _call(self, router, hs):
        return router(h_fine=hs[-1], h_coarse=hs[0]) if self.nb == 2 else router(h_fine=hs[2], h_median=hs[1], h_coarse=hs[0])

    def names(self):
        return BRANCH_NAMES[self.nb] + [n for n, _ in self.router.named_parameters()]


def _collect(out, grads, names):
    res = {k: out[k].detach() for k in ("h", "indices", "codebook_mask", "gate")}
    res["grads"] = {n: g.detach() for n, g in zip(names, grads)}
    return res


def reference64(inp):
    """the float64 statement of the op on the CPU: outputs and the gradients of sum(h R) + sum(gate Q)"""
    hs = [h.detach().double().requires_grad_(True) for h in inp.hs]
    r64 = Router64(inp.router.state_dict(), inp.nb, inp.geo["groups"], inp.geo["act"])
    gum = None if inp.gumbels is None else inp.gumbels.double()
    out = torch_tail(r64, hs, gum, inp.nb, inp.update_router, inp.tau)
    loss = (out["h"] * inp.R.double()).sum() + (out["gate"] * inp.Q.double()).sum()
    named = dict(r64.named())
    pn = [n for n, _ in inp.router.named_parameters()]
    grads = torch.autograd.grad(loss, hs + [named[n] for n in pn])
    return _collect(out, grads, inp.names())


def _on(inp, dev):
    router = copy.deepcopy(inp.router).to(dev)
    hs = [h.detach().to(dev).requires_grad_(True) for h in inp.hs]
    gum = None if inp.gumbels is None else inp.gumbels.to(dev)
    return router, hs, gum, inp.R.to(dev), inp.Q.to(dev)


def run_torch32(inp, dev):
    """the package's own fp32 torch-op chain (the router module's forward under autograd + torch_tail) on `dev`"""
    router, hs, gum, R, Q = _on(inp, dev)
    out = torch_tail(router, hs, gum, inp.nb, inp.update_router, inp.tau)
    loss = (out["h"] * R).sum() + (out["gate"] * Q).sum()
    grads = torch.autograd.grad(loss, hs + list(router.parameters()))
    return _collect(out, grads, inp.names())


def kernel_graph(inp, dev):
    """route_train_dual / route_train_triple on `dev` -> (outputs, the loss sum(h R) + sum(gate Q), the leaves in names() order)"""
    router, hs, gum, R, Q = _on(inp, dev)
    if inp.nb == 2:
        out = route_train_dual(router, hs[1], hs[0], tau=inp.tau, gumbels=gum, update_router=inp.update_router)
        out["h"] = out["h_dual"]
    else:
        out = route_train_triple(router, hs[2], hs[1], hs[0], tau=inp.tau, gumbels=gum)
        out["h"] = out["h_triple"]
    return out, (out["h"] * R).sum() + (out["gate"] * Q).sum(), hs + list(router.parameters())


def run_kernel(inp, dev):
    out, loss, leaves = kernel_graph(inp, dev)
    return _collect(out, torch.autograd.grad(loss, leaves), inp.names())


@functools.lru_cache(maxsize=None)
def case(i, tau=None):
    """(Inputs, float64 reference) of row i of CASES (i = -1: CASE_NO_UPDATE), computed once and shared; read-only"""
    if i < 0:
        inp = Inputs(CASE_NO_UPDATE, SEED_NO_UPDATE, update_router=False)
    else:
        inp = Inputs(CASES[i], i, tau=tau)                 # the row's index is its seed
    return inp, reference64(inp)


# ---- the slice rule -----------------------------------------------------------------------------------------------------------
def slices(t):
    """max |t| per slice: per (image, channel) plane of a 4-d tensor, per row of a matrix, over a whole vector"""
    a = t.detach().abs().double().cpu()
    if a.dim() == 4:
        return a.amax((2, 3)).flatten()
    if a.dim() == 2:
        return a.amax(1)
    return a.amax().reshape(1)


def slice_errors(got, t32, ref):
    """per slice: (err_kernel, err_torch32, floor) against the float64 `ref`"""
    ref = ref.detach().double().cpu()
    ek = slices(got.detach().double().cpu() - ref)
    et = slices(t32.detach().double().cpu() - ref)
    return ek, et, FLOOR_ROUNDINGS * U * slices(ref)


def m_needed(ek, et, floor):
    """the smallest m with err_kernel <= m err_torch32 + floor on every slice (inf where torch is exact and the floor is missed)"""
    over = (ek - floor).clamp(min=0.0)
    r = torch.where(over > 0, over / et, torch.zeros_like(over))
    return float(r.max()) if r.numel() else 0.0


def accuracy_record(inp, ref, ker, t32):
    """{tensor: {err_kernel, err_torch32, ratio, m_needed, max_ref}}: the tensor-wide maxima of both errors, their ratio, and the
    m the slice rule needs"""
    rec = {}
    items = list(ref["grads"].items())
    if not inp.update_router:
        items.append(("gate", ref["gate"]))
    for name, r in items:
        got = ker["gate"] if name == "gate" else ker["grads"][name]
        t = t32["gate"] if name == "gate" else t32["grads"][name]
        ek, et, fl = slice_errors(got, t, r)
        k, tt = float(ek.max()), float(et.max())
        rec[name] = {"err_kernel": k, "err_torch32": tt, "ratio": (k / tt if tt > 0 else (math.inf if k > 0 else 0.0)),
                     "m_needed": m_needed(ek, et, fl), "max_ref": float(r.abs().max())}
    return rec
