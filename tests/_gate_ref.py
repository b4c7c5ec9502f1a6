"""The fused feature-router gate (csrc/router_gate.hip, fused_router_gate / dvq_router_gate_f32) restated for its tests:

  * CASES: one row per edge of the kernels, each naming the edge it is there for, at the smallest shape that reaches it;
  * dispatch(): the host arithmetic of dvq_launch_router_gate in Python, written from the .hip text, as a function of the device's
    CU count -- which form runs (GEMM or direct), which instantiation, the ring chunking, the spread of cell blocks over
    workgroups, the pooling forms, the LDS bytes of the direct form, the workspace and prep sizes;
  * the reference: Router64 of tests/_route_train_ref.py (the routers' formula in float64 on the CPU, from the state dict of the
    module under test) and, as the fp32 yardstick, the module's own torch-op forward with grad enabled;
  * the rule: per image, err_kernel <= M * err_torch32 + 16 * 2^-24 * max |ref over the image|, and the argmax of float64 on every
    cell whose float64 top-2 margin exceeds twice that bound.
Nothing here calls the code under test except run_kernel."""
import copy
import functools

import torch

from tests import _route_train_ref as R

U = R.U
FLOOR_ROUNDINGS = R.FLOOR_ROUNDINGS
# The factor of the rule: twice the worst m any image of any row but the offset row needs, rounded up to an integer; at most 8
# (hi / lo operands carry 22 significand bits and lo * lo is dropped: products good to 2^-22 against fp32's 2^-24, a factor of 4;
# another summation order, a factor of 2).  Measured on an MI355X (profiles/router_gate_accuracy.json,
# tools/router_gate_accuracy.py) the worst m needed is 0 in every form -- direct <2,1>, <2,2>, <3,1>, tiled and untiled, the single
# Linear, gemm <2,8>, <2,24> PIPE, <2,32> PIPE, <3,24>: no image of any row leaves the sixteen-rounding floor, the kernel sits at
# 0.11 - 0.54 of it (largest: r09, gemm <2,32> PIPE, and r07, gemm <2,24> PIPE; the fp32 torch chain: 0.10 - 1.35 of it), so the
# rule is the floor alone.  The offset row would need m = 2.64 (6.7 floors, torch 2.7): it is not under the rule.
M = 0.0
OLD_BAR = 1e-4                                       # tests/test_gpu_parity.py: err < 1e-4 * max(1, max |ref|) over the whole tensor

ACT = {"1layer-fc": 0, "2layer-fc-SiLu": 1, "2layer-fc-ReLu": 2}
SILU, RELU, ONE = "2layer-fc-SiLu", "2layer-fc-ReLu", "1layer-fc"

# (name, nb, B, C, hc, wc, norm, gate_type, hidden or None (= F), seed, offsets or None, edge)
CASES = [
    ("r01", 2, 1, 8, 1, 2, "none", SILU, None, 1, None, "S = 1; one cell block of 2 cells; red exactly fills the tile area"),
    ("r02", 3, 2, 8, 3, 4, "group-2", RELU, None, 2, None, "F = 24, Fp = 32, S = 2: padded k, untiled loop"),
    ("r03", 3, 2, 40, 2, 6, "group-5", SILU, 72, 3, None,
     "F = 120, Fp = 128; hidden % 32 = 8; coarse pooled scalar, median / fine vector"),
    ("r04", 3, 3, 72, 4, 4, "none", ONE, None, 4, None, "F = 216, Fp = 224; single Linear over padded features"),
    ("r05", 2, 3, 64, 5, 6, "group-8", SILU, 16, 5, None,
     "GEMM <2,8>; one row tile, half masked; three idle waves per hidden group"),
    ("r06", 2, 3, 64, 5, 6, "group-8", SILU, 200, 6, None, "GEMM; HG = 2; last group has a !tile_ok wave"),
    ("r07", 2, 2, 192, 4, 4, "group-24", SILU, None, 7, None, "GEMM <2,24>, PIPE, one cell block exactly"),
    ("r08", 3, 2, 128, 3, 5, "group-16", RELU, None, 8, None, "GEMM <3,24>, ragged last block"),
    ("r09", 2, 35, 256, 7, 9, "group-32", SILU, None, 9, None,
     "GEMM <2,32> PIPE; 69 blocks over CG = 64: nmine 1 and 2 in one launch; last block partial"),
    ("r10a", 2, 2, 64, 24, 32, "group-8", SILU, None, 10, None, "at the 48 KiB pooling-LDS limit: GEMM form"),
    ("r10b", 2, 2, 64, 25, 32, "group-8", SILU, None, 10, None, "one row past the 48 KiB pooling-LDS limit: direct form"),
    ("r11", 2, 2, 32, 4, 4, "none", SILU, 3200, 11, None, "direct form: 100 row tiles over 8 waves; the LDS fits"),
    ("r12", 2, 2, 64, 4, 4, "group-8", SILU, 3200, 12, None,
     "GEMM form: HG * 4 = 100 slices, finalize's second and later rounds of 24"),
    ("r13", 2, 69, 8, 16, 15, "none", SILU, None, 13, None, "cb2: >= 64 cells per CU, ragged last workgroup, odd row length"),
    ("r14", 2, 257, 64, 16, 16, "group-8", SILU, None, 14, None, "fine branch > 64 MiB: gate_pool_kernel<true,true>"),
    ("r15", 2, 257, 64, 16, 16, "none", SILU, None, 15, None, "gate_pool_kernel<false,true> together with cb2"),
    ("r16", 2, 3, 64, 5, 6, "group-8", SILU, None, 16, (8.0, 64.0),
     "features + 8 and + 64 standard deviations of offset, per channel group"),
    ("r17", 2, 2, 96, 3, 3, "group-12", SILU, None, 17, None,
     "S16 = 12 has no two-branch GEMM instantiation: whole-octet groups take the direct form"),
]
NAMES = [c[0] for c in CASES]
ROW_OFFSET = "r16"                                   # held to the old bar and the argmax condition only
ABI_ROWS = ["r02", "r06", "r08", "r09", "r13"]       # dvq_router_gate_f32 called directly
NAN_ROWS = ["r03", "r06"]


def row(name):
    return CASES[NAMES.index(name)]


def groups_of(norm):
    return R.groups_of(norm)


# ---- the host arithmetic of router_gate.hip, restated ---------------------------------------------------------------------------
CACHED_MAX_BYTES = 64 << 20                          # dvq_common.h: DVQ_CACHED_MAX_BYTES
GATE_LDS_MAX = 160 * 1024 - 256                      # launchers.h: DVQ_GATE_LDS_MAX
GATE_NW = 8
GEMM_STEPS = {2: (8, 16, 24, 32), 3: (12, 24, 48)}   # the instantiations of gate_gemm_kernel<G, S>


def a256(x):
    return (x + 255) // 256 * 256


def hid_of(nb, C, gate_type, hidden):
    """the launcher's Hid: 32 for the single-layer gate"""
    return 32 if gate_type == ONE else (hidden if hidden is not None else nb * C)


def img_bytes(nb, C, Hid):
    Fp = (nb * C + 15) // 16 * 16
    return a256((Hid + 31) // 32 * 32 * Fp * 2 * 2)


def prep_bytes(nb, C, Hid):
    return img_bytes(nb, C, Hid) + 256


def ximg_bytes(nb, B, C, hc, wc):
    return a256((B * hc * wc + 31) // 32 * ((nb * C + 15) // 16) * 2048)


def part_bytes(nb, B, hc, wc, Hid):
    return a256((Hid + 127) // 128 * 4 * B * hc * wc * nb * 4)


def ws_bytes(nb, B, C, hc, wc, Hid):
    pool = a256(B * nb * C * hc * wc * 4)
    return (a256(B * nb * C * 8) + max(pool, ximg_bytes(nb, B, C, hc, wc)) + img_bytes(nb, C, Hid) + 256
            + part_bytes(nb, B, hc, wc, Hid) + 512)


def gemm_form(nb, C, hc, wc, groups, act):
    F = nb * C
    cpg = C // groups if groups > 0 else 0
    return (act != 0 and groups > 0 and cpg % 8 == 0 and cpg <= 64 and nb * cpg * hc * wc * 4 <= 48 * 1024 and F % 16 == 0
            and F // 16 in GEMM_STEPS[nb])


def direct_lds_bytes(nb, C, hc, wc, groups, Hid, act):
    """dynamic LDS of router_gate_kernel at one block of 32 cells; 0 for a shape that takes the GEMM form"""
    if gemm_form(nb, C, hc, wc, groups, act):
        return 0
    Fp = (nb * C + 15) // 16 * 16
    return (32 * Fp + (1 + nb) * Hid) * 4


def dispatch(case, ncu=256):
    """every quantity dvq_launch_router_gate and its kernels branch or tile on, for one row on a device of ncu CUs"""
    name, nb, B, C, hc, wc, norm, gate_type, hidden, seed, offsets, edge = case
    groups, act = groups_of(norm), ACT[gate_type]
    F = nb * C
    Fp = (F + 15) & ~15
    Hid = hid_of(nb, C, gate_type, hidden)
    ncell = B * hc * wc
    fs = 1 << (nb - 1)
    d = dict(name=name, nb=nb, B=B, C=C, hc=hc, wc=wc, groups=groups, act=act, F=F, Fp=Fp, S=Fp // 16, Hid=Hid, T=(Hid + 31) // 32,
             ncell=ncell, hidden_arg=0 if act == 0 else Hid,
             cached=B * C * hc * fs * wc * fs * 4 <= CACHED_MAX_BYTES,
             vec=[((wc << i) & 3) == 0 for i in range(nb)],          # pooling: 16-B loads where the rows are whole float4s
             cpg=C // groups if groups > 0 else 8, pool_groups=groups if groups > 0 else C // 8,
             gemm_form=gemm_form(nb, C, hc, wc, groups, act),
             ws_bytes=ws_bytes(nb, B, C, hc, wc, Hid), prep_bytes=prep_bytes(nb, C, Hid),
             lds=direct_lds_bytes(nb, C, hc, wc, groups, Hid, act))
    if d["gemm_form"]:
        S16 = F // 16
        CH = 16 if S16 % 16 == 0 else (8 if S16 % 8 == 0 else 4)
        nblocks = (ncell + 31) // 32
        HG = (Hid + 127) // 128
        CG = max(1, min(ncu // HG, nblocks))
        d.update(S16=S16, CH=CH, NCH=S16 // CH, RING=4 if CH == 16 else 8, PIPE=nb == 2 and S16 >= 20, HG=HG, CG=CG, nblocks=nblocks,
                 nmine=sorted({(nblocks - x + CG - 1) // CG for x in range(CG)}), memset=(ncell & 31) != 0,
                 idle_waves=HG * 4 - d["T"], pool_lds=nb * d["cpg"] * hc * wc * 4, pool_kernel=(True, not d["cached"]))
    else:
        shmem2 = (2 * 32 * Fp + (1 + nb) * Hid) * 4
        cb2 = act != 0 and shmem2 <= GATE_LDS_MAX - 256 and ncell >= 64 * ncu
        per = 64 if cb2 else 32
        d.update(cb2=cb2, grid=(ncell + per - 1) // per, shmem=shmem2 if cb2 else d["lds"], pipelined=(d["S"] & 3) == 0,
                 tiles_per_wave=(d["T"] + GATE_NW - 1) // GATE_NW, last_cells=ncell - (ncell - 1) // per * per,
                 pool_kernel=(False, not d["cached"]))
    return d


def abi_size_args(d, B=None):
    """(num_branches, B, C, hc, wc, num_groups, hidden) as dvq_router_gate_workspace_bytes takes them"""
    return d["nb"], d["B"] if B is None else B, d["C"], d["hc"], d["wc"], d["groups"], d["hidden_arg"]


# ---- one row: inputs, the float64 reference, the two fp32 evaluations -------------------------------------------------------------
class Inputs:
    """fp32 inputs of one row on the CPU: the module under test (eval mode) and the branches coarse -> fine; `logits64` are
    Router64's on the same values"""

    def __init__(self, case, seed=None):
        name, nb, B, C, hc, wc, norm, gate_type, hidden, row_seed, offsets, edge = case
        seed = row_seed if seed is None else seed
        self.case, self.nb, self.geo = case, nb, dispatch(case)
        cpu = torch.device("cpu")
        self.router = R.make_router(nb, C, norm, gate_type, cpu, 100 + seed, hidden).eval()
        self.hs = [h.detach() for h in R.branches(nb, B, C, hc, wc, cpu, 200 + seed)]
        if offsets is not None:                      # a large mean against the spread, another one per channel group
            G = self.geo["pool_groups"]
            for i, h in enumerate(self.hs):
                off = torch.tensor([offsets[g % len(offsets)] for g in range(G)]).repeat_interleave(C // G) * (0.5 + i)
                h.add_(off[None, :, None, None])
        self.logits64 = reference64(self)

    def call(self, router, hs):
        return router(h_fine=hs[-1], h_coarse=hs[0]) if self.nb == 2 else router(h_fine=hs[2], h_median=hs[1], h_coarse=hs[0])


def reference64(inp, router=None):
    """the float64 logits on the CPU, from the state dict of `router` (default: the row's own module)"""
    r = inp.router if router is None else router
    r64 = R.Router64(r.state_dict(), inp.nb, inp.geo["groups"], inp.geo["act"])
    with torch.no_grad():
        return inp.call(r64, [h.double() for h in inp.hs])


def on(inp, dev):
    return copy.deepcopy(inp.router).to(dev), [h.to(dev) for h in inp.hs]


def run_torch32(inp, dev, router=None, hs=None):
    """the module's own fp32 torch-op forward (grad enabled: its parameters require grad) on `dev`"""
    if router is None:
        router, hs = on(inp, dev)
    with torch.enable_grad():
        out = inp.call(router, hs)
    assert out.requires_grad, "the torch-op path was not taken"
    return out.detach()


def run_kernel(inp, dev, router=None, hs=None):
    """the fused kernel: the module under no_grad on `dev`"""
    if router is None:
        router, hs = on(inp, dev)
    with torch.no_grad():
        out = inp.call(router, hs)
    assert not out.requires_grad
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs (with the float64 logits) of a row, computed once and shared; read-only"""
    return Inputs(row(name))


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
def image_errors(got, t32, ref):
    """per image: (err_kernel, err_torch32, floor) against the float64 `ref` [B, hc, wc, nb]"""
    ref = ref.detach().double().cpu()
    ek = (got.detach().double().cpu() - ref).abs().amax((1, 2, 3))
    et = (t32.detach().double().cpu() - ref).abs().amax((1, 2, 3))
    return ek, et, FLOOR_ROUNDINGS * U * ref.abs().amax((1, 2, 3))


def clear_cells(ref, et, floor, m=None):
    """[B, hc, wc] bool: the float64 top-2 margin exceeds 2 * (m * err_torch32 + floor) of the cell's image -- two logits each
    within E of the truth can swap only inside a margin of 2 E"""
    thr = 2.0 * ((M if m is None else m) * et + floor)
    return R.margin(ref.detach().double().cpu()) > thr[:, None, None]


def check_rule(got, t32, ref, slice_rule=True, label=""):
    """rule (a) on one evaluation; prints each figure before it asserts.  -> the m the slice rule needs"""
    assert tuple(got.shape) == tuple(ref.shape), (tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), label + ": a logit is not finite"
    ek, et, fl = image_errors(got, t32, ref)
    need = R.m_needed(ek, et, fl)
    top = float(ref.abs().max())
    print("%s err_kernel %.3g err_torch32 %.3g max|ref| %.3g m needed %.3g" % (label, float(ek.max()), float(et.max()), top, need))
    bad = []
    if slice_rule:
        fail = (ek > M * et + fl).nonzero().flatten().tolist()
        if fail:
            j = fail[0]
            bad.append("%d images, first %d: err_kernel %.3g > %g * %.3g + %.3g" % (len(fail), j, float(ek[j]), M, float(et[j]),
                                                                                    float(fl[j])))
    if float(ek.max()) >= OLD_BAR * max(1.0, top):
        bad.append("%.3g beyond 1e-4 * max(1, max |ref|) = %.3g" % (float(ek.max()), OLD_BAR * max(1.0, top)))
    clear = clear_cells(ref, et, fl)
    wrong = int((got.detach().cpu().argmax(-1) != ref.argmax(-1))[clear].sum())
    if wrong:
        bad.append("argmax differs from float64's on %d of %d clear cells" % (wrong, int(clear.sum())))
    assert not bad, label + ": " + "; ".join(bad)
    return need


def accuracy_record(got, t32, ref):
    """per image: both errors, their ratio and the m the rule needs"""
    ek, et, fl = image_errors(got, t32, ref)
    over = (ek - fl).clamp(min=0.0)
    m = torch.where(over > 0, over / et, torch.zeros_like(over))
    ratio = torch.where(et > 0, ek / et, torch.where(ek > 0, torch.full_like(ek, float("inf")), torch.zeros_like(ek)))
    return {"err_kernel": ek.tolist(), "err_torch32": et.tolist(), "ratio": ratio.tolist(), "m_needed": m.tolist(),
            "max_ref": (fl / (FLOOR_ROUNDINGS * U)).tolist(), "worst_m_needed": float(m.max())}
