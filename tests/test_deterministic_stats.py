"""Bit-reproducible per-code sums: dvq_code_sums_det / dvq_vq_backward_codebook_det_f32 and the `set_deterministic` switch.

The summation order is documented in include/dvq.h; tests/_det_stats_ref.py restates it in numpy float32 and the GPU tests ask for
BIT equality with that restatement -- sums, gradient and counts -- at shapes that cross every path of the kernels (a partial tile, one
token in a second tile, segments longer than the long-segment threshold, more codes than a tile has tokens, widths that are no
multiple of the 16-channel slice, NCHW maps with HW % 4 != 0 and == 0, rows, float32 / fp16 / bf16).  Bounds: equality needs none; the
restatement itself is held to the project's 1e-5-of-the-largest-entry criterion against a float64 scatter-add on the CPU."""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import _det_stats_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dvq_code_sums_det_workspace_bytes", "dvq_code_sums_det", "dvq_vq_backward_codebook_det_workspace_bytes",
       "dvq_vq_backward_codebook_det_f32")
ATOMIC = {"dvq_ema_accumulate_nchw_f32", "dvq_ema_accumulate_nchw_x16", "dvq_vq_backward_codebook_nchw_f32"}
DET = {"dvq_code_sums_det", "dvq_vq_backward_codebook_det_f32"}


# ---------------------------------------------------------------- CPU -----------------------------------------------------------
def test_the_symbols_are_declared_and_exported_and_the_version_stays():
    from dynamicvectorquantization_amd import _lib
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name), name
    assert _lib.lib.dvq_version() == 2000
    header = open(os.path.join(ROOT, "include", "dvq.h")).read()
    assert "enum { DVQ_DET_TILE = %d, DVQ_DET_RUN = %d, DVQ_DET_MAX_K = 16384 };" % (R.TILE, R.RUN) in header
    assert (_lib.DET_TILE, _lib.DET_RUN, _lib.DET_MAX_K) == (R.TILE, R.RUN, 16384)
    q = _lib.lib.dvq_code_sums_det_workspace_bytes
    assert q(256, 256, 1024, 1024) == _lib.lib.dvq_vq_backward_codebook_det_workspace_bytes(256, 256, 1024, 1024) > 128 * 1024 * 1024
    assert q(256, 256, 1024, 1024) % 256 == 0
    assert q(1, 4, 1, 16385) == 0 and q(1, 6, 1, 8) == 0 and q(0, 4, 1, 8) == 0 and q(1, 4, 1, 16384) > 0


def test_the_validation_rows_of_the_new_calls_replay_without_a_gpu():
    """every refusal tests/golden/abi_rejections_det.json records for the two calls, replayed as tests/test_abi_rejections.py replays
    its table: by tools/gen_golden_abi_rejections.py --replay in a child process that sees no GPU, so that a check a later edit
    loses shows as a wrong rc and never as a kernel on the fake pointers.  The two are ordinary status calls; their rows stand in a
    table of their own (written by the same tool in the same run) because tests/golden/abi_rejections.json is kept as it was, and
    `_lib._TABLED_APART` names exactly them."""
    import json
    import subprocess
    import sys
    from dynamicvectorquantization_amd import _lib
    table = os.path.join(ROOT, "tests", "golden", "abi_rejections_det.json")
    rows = json.load(open(table))
    assert {r["fn"] for r in rows} == DET == set(_lib._TABLED_APART) and len(rows) >= 20
    for fn in DET:                                              # status calls like the rest: int, and checked.* raises
        assert _lib._PROTOTYPES[fn][0] is ctypes.c_int
        with pytest.raises(_lib.DvqError, match="null pointer"):
            getattr(_lib.checked, fn)(*([0] * len(_lib._PROTOTYPES[fn][1])))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    tool = os.path.join(ROOT, "tools", "gen_golden_abi_rejections.py")
    out = subprocess.run([sys.executable, tool, "--replay", table], env=env, check=True, capture_output=True, text=True, timeout=120).stdout
    got = json.loads(out)
    assert len(got) == len(rows)
    seen = set()
    for r, (rc, message) in zip(rows, got):
        assert r["rc"] in (-1, -2, -3), r
        assert (rc, message) == (r["rc"], r["message"]), (r["fn"], r["args"])
        seen.add((r["fn"], r["rc"]))
    for fn in DET:                                              # invalid, unsupported (naming the limit), workspace
        assert {(fn, -1), (fn, -2), (fn, -3)} <= seen
    assert any("16384" in r["message"] for r in rows if r["rc"] == -2)
    # the first table holds none of them and is the generator's first output, row for row
    assert not [r for r in json.load(open(os.path.join(ROOT, "tests", "golden", "abi_rejections.json"))) if r["fn"] in DET]


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=R.CASE_IDS)
def test_the_documented_order_meets_the_1e5_criterion_against_float64(i):
    v, codes = R.case_inputs(i)
    K = R.CASES[i][2]
    counts, sums = R.case_reference(i, "float32")
    c64, s64 = R.scatter_f64(v, codes, K)
    assert np.array_equal(counts, c64.astype(np.float32))
    assert np.abs(sums - s64).max() <= 1e-5 * np.abs(s64).max()
    assert not np.signbit(sums[c64 == 0]).any()                # a code without members: +0.0


def test_another_tile_or_run_length_gives_other_bits():
    """bit equality discriminates between summation orders: the restatement with another tile or run differs somewhere"""
    v, codes = R.case_inputs(4)
    K = R.CASES[4][2]
    _, base = R.case_reference(4, "float32")
    assert not np.array_equal(base, R.det_sums(v, codes, K, tile=1024)[1])
    assert not np.array_equal(base, R.det_sums(v, codes, K, run=16)[1])


@contextlib.contextmanager
def recording(monkeypatch):
    """the entry points the package asks `_lib.checked` for, in order, WITHOUT running them (no GPU): size queries answer 1 MiB"""
    from dynamicvectorquantization_amd import _lib
    names = []
    with monkeypatch.context() as m:
        for n in _lib.EXPORTS:
            m.setattr(_lib.checked, n, (lambda n: lambda *a: (names.append(n), (1 << 20) if n.endswith("_bytes") else 0)[1])(n))
        m.setattr(_lib, "stream_ptr", lambda device: 0)
        m.setattr(_lib, "on_device", lambda device: _lib._NO_SWITCH)
        yield names


def _fake(t):
    return t                                                    # (nothing is launched: plain CPU tensors carry the pointers)


def _dispatch(monkeypatch):
    from dynamicvectorquantization_amd import _lib
    z, codes = _fake(torch.zeros(8, 16)), _fake(torch.zeros(8, dtype=torch.int64))
    counts, sums = _fake(torch.zeros(4)), _fake(torch.zeros(4, 16))
    with recording(monkeypatch) as names:
        _lib.code_sums_into(z, codes, 8, 16, 1, 4, counts, sums)
        _lib.code_sums_into(_fake(torch.zeros(8, 16, dtype=torch.bfloat16)), codes, 8, 16, 1, 4, counts, sums)
    return [n for n in names if not n.endswith("_bytes")]


def test_set_deterministic_selects_the_entry_points(monkeypatch):
    import dynamicvectorquantization_amd as pkg
    assert not torch.are_deterministic_algorithms_enabled()
    prev = pkg.set_deterministic(None)
    try:
        assert _dispatch(monkeypatch) == ["dvq_ema_accumulate_nchw_f32", "dvq_ema_accumulate_nchw_x16"]       # None, torch's flag off
        pkg.set_deterministic(False)
        assert _dispatch(monkeypatch) == ["dvq_ema_accumulate_nchw_f32", "dvq_ema_accumulate_nchw_x16"]
        pkg.set_deterministic(True)
        assert _dispatch(monkeypatch) == ["dvq_code_sums_det", "dvq_code_sums_det"]
        pkg.set_deterministic(None)
        torch.use_deterministic_algorithms(True)
        try:
            assert pkg.is_deterministic() and _dispatch(monkeypatch) == ["dvq_code_sums_det", "dvq_code_sums_det"]   # None follows torch
            pkg.set_deterministic(False)
            assert _dispatch(monkeypatch) == ["dvq_ema_accumulate_nchw_f32", "dvq_ema_accumulate_nchw_x16"]       # the package's own choice wins
        finally:
            torch.use_deterministic_algorithms(False)
        with pytest.raises(TypeError):
            pkg.set_deterministic(1)
    finally:
        pkg.set_deterministic(prev)


def test_cpu_statistics_under_the_switch_stay_on_torch_and_agree(monkeypatch):
    """CPU tensors: bincount / index_add_ with torch's flag held on, never a kernel; the flag is put back"""
    import dynamicvectorquantization_amd as pkg
    from dynamicvectorquantization_amd.quantize import VQEmbedding
    emb = VQEmbedding(8, 4)
    x = torch.randn(40, 4, generator=torch.Generator().manual_seed(3))
    idx = torch.randint(0, 8, (40,), generator=torch.Generator().manual_seed(4))
    prev = pkg.set_deterministic(True)
    try:
        with recording(monkeypatch) as names:
            cs, vs, _ = emb._cluster_sums(x, idx)
        assert not names and not torch.are_deterministic_algorithms_enabled()
    finally:
        pkg.set_deterministic(prev)
    c64, s64 = R.scatter_f64(x.numpy(), idx.numpy(), 8)
    assert np.array_equal(cs.numpy(), c64.astype(np.float32)) and np.allclose(vs.numpy(), s64, rtol=0, atol=1e-5 * np.abs(s64).max())


# ---------------------------------------------------------------- GPU -----------------------------------------------------------
def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _layouts(i, v_t):
    """the case's tokens as (name, z, B, HW): an NCHW map with HW % 4 != 0, and rows"""
    N, D = v_t.shape
    B, HW = R.NCHW_OF[N]
    assert B * HW == N and HW % 4 != 0
    return [("nchw", v_t.reshape(B, HW, D).permute(0, 2, 1).contiguous(), B, HW), ("rows", v_t.contiguous(), N, 1)]


def _stats(z, codes, B, D, HW, K, ws=None):
    from dynamicvectorquantization_amd import _lib
    counts = torch.full((K,), -7.0, device=z.device)                     # both outputs are overwritten
    sums = torch.full((K, D), -7.0, device=z.device)
    ws = _lib.det_workspace(B, D, HW, K, z.device) if ws is None else ws
    _lib.checked.dvq_code_sums_det(z.data_ptr(), _lib.X16.get(z.dtype, 0), codes.data_ptr(), B, D, HW, K, counts.data_ptr(),
                                   sums.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(z.device))
    return counts, sums


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("i", range(len(R.CASES)), ids=R.CASE_IDS)
def test_statistics_equal_the_restatement_bit_for_bit(dev, i, dtype):
    v, codes = R.case_inputs(i)
    N, D, K, _ = R.CASES[i]
    want_counts, want_sums = R.case_reference(i, str(dtype).split(".")[1])
    v_t, c_t = torch.from_numpy(v).to(dtype).to(dev), torch.from_numpy(codes).to(dev)
    for name, z, B, HW in _layouts(i, v_t):
        counts, sums = _stats(z, c_t, B, D, HW, K)
        torch.cuda.synchronize()
        assert np.array_equal(counts.cpu().numpy(), want_counts), name
        got = sums.cpu().numpy()
        diff = got.view(np.int32) != want_sums.view(np.int32)
        assert not diff.any(), (name, int(diff.sum()), float(np.abs(got - want_sums).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("with_mask", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("i", range(len(R.CASES)), ids=R.CASE_IDS)
def test_codebook_gradient_equals_the_restatement_bit_for_bit(dev, i, with_mask):
    from dynamicvectorquantization_amd import _lib
    v, codes = R.case_inputs(i)
    N, D, K, _ = R.CASES[i]
    rng = np.random.default_rng(3000 + i)
    E = rng.standard_normal((K, D)).astype(np.float32)
    mask = rng.integers(0, 2, N).astype(np.float32) * np.float32(1.5) if with_mask else None
    g_loss, coef = np.float32(0.7), np.float32(2.0 / (N * D))
    want = R.det_grad(v, E, codes, mask, g_loss, coef)
    v_t, c_t, E_t = torch.from_numpy(v).to(dev), torch.from_numpy(codes).to(dev), torch.from_numpy(E).to(dev)
    m_t = None if mask is None else torch.from_numpy(mask).to(dev)
    gl = torch.tensor([float(g_loss)], device=dev)
    for name, z, B, HW in _layouts(i, v_t):
        gw = torch.full((K + 1, D), -7.0, device=dev)                    # rows 0 .. K - 1 are written, not accumulated into
        ws = _lib.det_workspace(B, D, HW, K, dev)
        _lib.checked.dvq_vq_backward_codebook_det_f32(z.data_ptr(), E_t.data_ptr(), c_t.data_ptr(), _lib.ptr(m_t), gl.data_ptr(),
                                                      float(coef), B, D, HW, K, gw.data_ptr(), ws.data_ptr(), ws.numel(),
                                                      _lib.stream_ptr(dev))
        torch.cuda.synchronize()
        got = gw.cpu().numpy()
        assert (got[K] == -7.0).all(), name
        diff = got[:K].view(np.int32) != want.view(np.int32)
        assert not diff.any(), (name, int(diff.sum()), float(np.abs(got[:K] - want).max()))


@pytest.mark.gpu
def test_codebook_gradient_at_every_load_form(dev):
    """the gradient on 4200 tokens as 42 x 100 (HW % 4 == 0: four tokens per load), 8 x 525 (element loads), aligned rows and rows one
    element off the allocation, with a mask: one result, the restatement's"""
    from dynamicvectorquantization_amd import _lib
    i = 6
    v, codes = R.case_inputs(i)
    N, D, K, _ = R.CASES[i]
    rng = np.random.default_rng(3100)
    E = rng.standard_normal((K, D)).astype(np.float32)
    mask = rng.integers(0, 2, N).astype(np.float32) * np.float32(0.75)
    g_loss, coef = np.float32(-1.3), np.float32(2.0 / (N * D))
    want = R.det_grad(v, E, codes, mask, g_loss, coef)
    v_t, c_t, E_t, m_t = (torch.from_numpy(a).to(dev) for a in (v, codes, E, mask))
    gl = torch.tensor([float(g_loss)], device=dev)
    off = torch.empty(N * D + 1, device=dev)[1:].view(N, D)
    off.copy_(v_t)
    assert off.data_ptr() % 16 != 0
    forms = [(v_t.reshape(B, HW, D).permute(0, 2, 1).contiguous(), B, HW) for B, HW in ((42, 100), (8, 525))] + [(v_t, N, 1), (off, N, 1)]
    for z, B, HW in forms:
        gw = torch.full((K, D), -7.0, device=dev)
        ws = _lib.det_workspace(B, D, HW, K, dev)
        _lib.checked.dvq_vq_backward_codebook_det_f32(z.data_ptr(), E_t.data_ptr(), c_t.data_ptr(), m_t.data_ptr(), gl.data_ptr(),
                                                      float(coef), B, D, HW, K, gw.data_ptr(), ws.data_ptr(), ws.numel(),
                                                      _lib.stream_ptr(dev))
        torch.cuda.synchronize()
        assert np.array_equal(gw.cpu().numpy().view(np.int32), want.view(np.int32)), (B, HW)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
def test_layout_and_factorisation_do_not_change_the_bits(dev, dtype):
    """4200 tokens as 8 x 525 (element loads), 42 x 100 (HW % 4 == 0: four tokens per load), rows (four channels per load), rows in a
    view one element off the allocation (element loads: what a C caller's unaligned z takes), and through the functional on a
    channels_last tensor: one result, the restatement's"""
    from dynamicvectorquantization_amd.quantize import code_sums
    i = 6
    v, codes = R.case_inputs(i)
    N, D, K, _ = R.CASES[i]
    want_counts, want_sums = R.case_reference(i, str(dtype).split(".")[1])
    v_t, c_t = torch.from_numpy(v).to(dtype).to(dev), torch.from_numpy(codes).to(dev)
    results = []
    for B, HW in ((8, 525), (42, 100)):
        z = v_t.reshape(B, HW, D).permute(0, 2, 1).contiguous()
        results.append(_stats(z, c_t, B, D, HW, K))
    results.append(_stats(v_t, c_t, N, D, 1, K))
    off = torch.empty(N * D + 1, dtype=dtype, device=dev)[1:].view(N, D)
    off.copy_(v_t)
    assert v_t.data_ptr() % (4 * v_t.element_size()) == 0 and off.data_ptr() % (4 * off.element_size()) != 0
    results.append(_stats(off, c_t, N, D, 1, K))
    cl = v_t.reshape(42, 10, 10, D).permute(0, 3, 1, 2)                   # channels_last [42, D, 10, 10]
    assert not cl.is_contiguous() and cl.is_contiguous(memory_format=torch.channels_last)
    results.append(code_sums(cl, c_t.reshape(42, 10, 10), K, deterministic=True))
    results.append(code_sums(v_t.reshape(42, 100, D).permute(0, 2, 1).contiguous().reshape(42, D, 10, 10), c_t, K, deterministic=True))
    for counts, sums in results:
        assert np.array_equal(counts.cpu().numpy(), want_counts)
        assert np.array_equal(sums.cpu().numpy().view(np.int32), want_sums.view(np.int32))
    # the atomic kernels give the same statistics to rounding (the existing criterion)
    counts, sums = code_sums(v_t, c_t, K, deterministic=False)
    assert np.array_equal(counts.cpu().numpy(), want_counts)
    assert np.abs(sums.cpu().numpy() - want_sums).max() <= 1e-5 * np.abs(want_sums).max()


@pytest.mark.gpu
def test_repeated_calls_on_one_workspace_and_a_graph_replay_give_the_same_bits(dev):
    from dynamicvectorquantization_amd import _lib
    i = 4
    v, codes = R.case_inputs(i)
    N, D, K, _ = R.CASES[i]
    _, want_sums = R.case_reference(i, "float32")
    z, c_t = torch.from_numpy(v).to(dev), torch.from_numpy(codes).to(dev)
    ws = _lib.det_workspace(N, D, 1, K, dev)
    first = None
    for _ in range(5):
        ws.fill_(0xA5 if first is None else 0x5A)                        # (what the workspace held does not matter)
        counts, sums = _stats(z, c_t, N, D, 1, K, ws)
        first = (counts, sums) if first is None else first
        assert _same_bits(counts, first[0]) and _same_bits(sums, first[1])
    assert np.array_equal(first[1].cpu().numpy().view(np.int32), want_sums.view(np.int32))
    counts = torch.empty(K, device=dev)
    sums = torch.empty(K, D, device=dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _lib.checked.dvq_code_sums_det(z.data_ptr(), 0, c_t.data_ptr(), N, D, 1, K, counts.data_ptr(), sums.data_ptr(), ws.data_ptr(),
                                       ws.numel(), _lib.stream_ptr(dev))
    for _ in range(2):
        counts.fill_(-1.0)
        sums.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bits(counts, first[0]) and _same_bits(sums, first[1])


def _train_three_steps(make, x, deterministic, seed=11):
    """a fresh module trained three steps on x (plain SGD on whatever has a gradient); -> (state_dict, x.grad of the last step)"""
    import dynamicvectorquantization_amd as pkg
    assert pkg.set_deterministic(None) is None
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    m = make().train()
    torch.use_deterministic_algorithms(deterministic)
    try:
        for step in range(3):
            xr = (x * (1.0 + 0.25 * step)).detach().requires_grad_(True)
            out = m(xr)
            w = torch.linspace(-1.0, 1.0, out[0].numel(), device=x.device).reshape(out[0].shape).to(out[0].dtype)
            ((out[0] * w).float().sum() + 3.0 * out[1]).backward()
            with torch.no_grad():
                for p in m.parameters():
                    if p.grad is not None:
                        p.add_(p.grad, alpha=-0.5)
                        p.grad = None
        torch.cuda.synchronize()
    finally:
        torch.use_deterministic_algorithms(False)
    return {k: t.detach().clone() for k, t in m.state_dict().items()}, xr.grad.detach().clone()


def _module_cases(dev):
    from dynamicvectorquantization_amd.quantize import EMAVectorQuantizer, MaskVectorQuantize, VectorQuantize2
    from dynamicvectorquantization_amd.rq import RQBottleneck
    g = torch.Generator().manual_seed(5)
    img = torch.randn(4, 64, 12, 12, generator=g).to(dev)                 # 576 tokens, D = 64
    return {
        "vq2_nchw_f32": (lambda: VectorQuantize2(48, 64).to(dev), img),
        "vq2_channels_last_bf16": (lambda: VectorQuantize2(48, 64).to(dev),
                                   img.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)),
        "rq_depth2": (lambda: RQBottleneck(latent_shape=(8, 8, 64), code_shape=(8, 8, 2), n_embed=64).to(dev),
                      torch.randn(3, 8, 8, 64, generator=g).to(dev)),
        "ema_vq": (lambda: EMAVectorQuantizer(48, 64, 0.25).to(dev), img),
        "maskvq_temp0": (lambda: MaskVectorQuantize(48, 64).to(dev), img),
    }


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["vq2_nchw_f32", "vq2_channels_last_bf16", "rq_depth2", "ema_vq", "maskvq_temp0"])
def test_modules_train_to_equal_bits_under_the_torch_flag(dev, name, monkeypatch):
    from dynamicvectorquantization_amd import _lib
    make, x = _module_cases(dev)[name]
    names = []
    for n in DET | ATOMIC:
        monkeypatch.setattr(_lib.checked, n, (lambda fn, n: lambda *a: (names.append(n), fn(*a))[1])(getattr(_lib.checked, n), n))
    a_state, a_grad = _train_three_steps(make, x, True)
    assert names and set(names) <= DET, names                            # only the fixed-order kernels ran
    b_state, b_grad = _train_three_steps(make, x, True)
    assert a_state.keys() == b_state.keys() and _same_bits(a_grad.float(), b_grad.float())
    for k in a_state:
        assert torch.equal(a_state[k], b_state[k]) and (not a_state[k].is_floating_point() or _same_bits(a_state[k].float(), b_state[k].float())), k
    del names[:]
    c_state, c_grad = _train_three_steps(make, x, False)                  # the float-atomic path: the same training, to rounding
    assert names and set(names) <= ATOMIC, names
    for k in a_state:
        if a_state[k].is_floating_point() and a_state[k].numel():
            a, c = a_state[k].float(), c_state[k].float()
            assert (a - c).abs().max() <= 1e-5 * c.abs().max().clamp_min(1e-30), k
    # x.grad of the last step reads the codebook the two earlier updates wrote.  float32: the same criterion.  A bfloat16 gradient is
    # the float32 value rounded once to 8 significant bits, and a 1e-7 difference of the codebook can move an entry across a rounding
    # boundary: such an entry may differ by ONE step of its own grid, 2^-7 of its own size (plus the float32 criterion as the floor for
    # entries near zero), never more; and it is rare -- a boundary lies within 1e-7 of a value with probability about 1e-7 / 2^-8 =
    # 3e-5 -- so at least 99.9 % of the entries must be equal bit for bit (30 times the expected share may differ).
    a, c = a_grad.float(), c_grad.float()
    floor = 1e-5 * c.abs().max()
    if x.dtype == torch.float32:
        assert (a - c).abs().max() <= floor
    else:
        assert bool(((a - c).abs() <= 2.0 ** -7 * c.abs() + floor).all()), float(((a - c).abs() - 2.0 ** -7 * c.abs()).max())
        assert float((a == c).float().mean()) >= 0.999, float((a == c).float().mean())
