"""The code exchange's pack and unpack kernels (csrc/exchange.hip) away from the benchmark's grid: ragged worlds, ranks without an
image, the int32 wire type and the int16 edge, sections whose length is no multiple of 8, more grain indices than codes, and loops
that live on their grid stride.  The format is restated in tests/_exchange_ref.py (numpy, nothing shared with the package); every
comparison is exact: bytes, int64 values, and the bits of the float32 mean (rank-order float64 sums, one division, one rounding).

  case  world  batch  cpi   gpi   num_codes  what it reaches
  a     1      1      1     0     2          smallest; no grain; nbytes == 24
  b     2      5      3     1     32768      ragged; both paddings non-empty; int16 edge (32767 travels)
  c     3      2      5     7     32769      empty last rank; first int32 size (32768 travels)
  d     8      13     16    4     1024       extra = 5, base = 1
  e     8      8      16    4     1024       even control
  f     5      4      2     3     100        base = 0, extra = 4
  g     16     3      2     1     10         13 empty ranks
  h     3      7      1     4096  100000     pack grid of one workgroup: the grain loop on its grid stride; int32 (99999 travels)
  i     1      520    1024  256   1024       b_max cpi = 532480 > 2048 * 256: pack and unpack code loops on their grid stride
  j     3      1563   341   85    40000      the same for the unpack at world 3, int32 (1563 = 3 * 521: an even split)
  l     3      1564   341   85    40000      j with one image more: grid stride, ragged and int32 together
  k     7      100    1024  256   1024       the workload's own grid, ragged

`test_case_table_reaches_what_it_claims` checks the last column without a device.  Codes are uniform in [0, num_codes) with
num_codes - 1 and 0 forced into the first and last element of every non-empty shard; grain indices are in {0, 1, 2}; every non-empty
rank has a local mean of its own; empty ranks pass no loss and null pointers.

On the GPU a world of W ranks is one process: rank r is packed straight into gathered[r nbytes : (r + 1) nbytes] of one allocation
prefilled with 0xA5 and followed by 64 guard bytes, the outputs of the unpack are followed by 16 sentinel elements.  One test runs
three rank processes on the one device (gloo rendezvous) for what only `CodeExchange` itself does: its pointers for an empty shard,
its buffers, the collective between the two kernels.

What the cases see.  Single-token changes of exchange.hip whose every access stays inside the test's allocations were tried on a
scratch build; the in-process GPU tests that fail, by case ("bytes" is the pack-and-unpack test of every case, "k>t" and "r>k" the
two cross-format tests on b, c, d):

  the wire-type threshold `<= 32768` read as `<= 65536`   bytes c, j, l; k>t c; r>k c; the stale-loss test on c.  dvq_exchange_bytes
                                                          then disagrees with the reference and the test stops before any launch;
                                                          h (100000 codes) stays int32 and passes
  the mean loop starting at rank 1                        bytes of all twelve cases (a: an empty sum, NaN); r>k b, c, d; the
                                                          null-grain test; the stale-loss tests (k>t passes: there torch adds the pairs)
  `pair[1]` written as 1                                  bytes of all twelve cases; k>t b, c, d; null grain; stale loss
  `pair[0]` without `* numel`                             the same tests as the line above
  `numel != 0.0` dropped from the pair's condition        the two stale-loss tests only (c, g): no other test hands an empty rank a loss
  `start = r * base`, the `extra` term dropped            run on b and l alone, where extra == 1 and the shifted read ends inside the
                                                          rank's own code section: bytes b, l; r>k b.  (Where extra > 1 the last rank
                                                          would read past the gathered buffer: not run.)

The kernels as they were before this file (padding bytes left as found, null pointers of an empty shard refused, no grain zero-fill
without a grain pointer, `loss[0] * 0` for an empty rank): bytes a, b, e, h, j, l and the no-loss test fail on the 0xA5 that the
padding keeps; bytes c, f, g, k>t c, both stale-loss tests and rank 2 of the three-process test end in "dvq_exchange_pack: null
pointer"; d, i, k (no padding, no empty rank) pass.
"""
import collections
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from dynamicvectorquantization_amd import _lib
from dynamicvectorquantization_amd.encode import _pack_torch, _unpack_torch, shard_slice
from tests import _exchange_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

Case = collections.namedtuple("Case", "world batch cpi gpi num_codes")
CASES = {
    "a": Case(1, 1, 1, 0, 2),
    "b": Case(2, 5, 3, 1, 32768),
    "c": Case(3, 2, 5, 7, 32769),
    "d": Case(8, 13, 16, 4, 1024),
    "e": Case(8, 8, 16, 4, 1024),
    "f": Case(5, 4, 2, 3, 100),
    "g": Case(16, 3, 2, 1, 10),
    "h": Case(3, 7, 1, 4096, 100000),
    "i": Case(1, 520, 1024, 256, 1024),
    "j": Case(3, 1563, 341, 85, 40000),
    "l": Case(3, 1564, 341, 85, 40000),
    "k": Case(7, 100, 1024, 256, 1024),
}
NAMES = tuple(CASES)
CROSS = ("b", "c", "d")
GUARD_BYTES, GUARD = 64, 16
FILL = 0xA5
SENT = -0x5A5A5A5A5A5A5A5B          # no code and no grain index is negative
SENT_F = 12345.0

Inputs = collections.namedtuple("Inputs", "case L b_max shards npi codes grain loss numel g_codes g_grain bufs mean")


def make_inputs(case, seed, with_loss=True):
    """Per rank: codes [b_local, cpi] int64, grain [b_local, gpi] int64 or None, the local mean (float32, None on an empty rank
    or with with_loss=False) and the element count; the global tensors; the reference buffers and the reference mean."""
    case = Case(*case)
    W, B, cpi, gpi, K = case
    rng = np.random.default_rng(seed)
    b_max = ref.b_max_of(B, W)
    L = ref.layout(cpi, gpi, b_max, K)
    shards = [ref.shard(B, r, W) for r in range(W)]
    npi = 3 * cpi                                               # elements of the loss numerator per image
    codes, grain, loss, numel, bufs = [], [], [], [], []
    for start, size in shards:
        c = rng.integers(0, K, size=(size, cpi), dtype=np.int64)
        if size:
            c.reshape(-1)[0], c.reshape(-1)[-1] = K - 1, 0
            if c.size == 1:                                     # one element cannot be both: the largest code travels
                c.reshape(-1)[0] = K - 1
        g = rng.integers(0, 3, size=(size, gpi), dtype=np.int64) if gpi else None
        m = np.float32(0.5 + rng.random()) if (size and with_loss) else None
        codes.append(c); grain.append(g); loss.append(m); numel.append(float(size * npi))
        bufs.append(ref.pack(c, g, m, numel[-1], b_max, K))
    g_codes = np.concatenate(codes, 0)
    g_grain = np.concatenate(grain, 0) if gpi else None
    u_codes, u_grain, mean = ref.unpack(np.concatenate(bufs), W, B, cpi, gpi, K)
    assert np.array_equal(u_codes, g_codes) and (gpi == 0 or np.array_equal(u_grain, g_grain))     # the reference inverts itself
    for a in codes + bufs + [g_codes] + ([g_grain] + grain if gpi else []):
        a.setflags(write=False)
    return Inputs(case, L, b_max, shards, npi, codes, grain, loss, numel, g_codes, g_grain, bufs, mean)


_CACHE = {}


def _inputs(name, with_loss=True):
    """computed once per case, shared by the tests and never written to afterwards"""
    key = (name, with_loss)
    if key not in _CACHE:
        _CACHE[key] = make_inputs(CASES[name], 1000 + NAMES.index(name), with_loss)
    return _CACHE[key]


def _bits(x):
    return int(np.asarray(x, dtype=np.float32).reshape(-1)[:1].view(np.uint32)[0])


def _xch_grid(items):
    return min(2048, max(1, -(-items // 256)))


# ---- CPU --------------------------------------------------------------------------------------------------------------------

def test_case_table_reaches_what_it_claims():
    shards = {n: [ref.shard(c.batch, r, c.world)[1] for r in range(c.world)] for n, c in CASES.items()}
    lay = {n: ref.layout(c.cpi, c.gpi, max(shards[n]), c.num_codes) for n, c in CASES.items()}
    pad = {n: (lay[n].off_grain - max(shards[n]) * CASES[n].cpi * lay[n].esize,
               lay[n].off_pair - lay[n].off_grain - max(shards[n]) * CASES[n].gpi) for n in CASES}
    for n, c in CASES.items():
        assert sum(shards[n]) == c.batch and max(shards[n]) == ref.b_max_of(c.batch, c.world)
    assert lay["a"].nbytes == 24 and CASES["a"].gpi == 0
    assert shards["b"] == [3, 2] and min(pad["b"]) > 0 and lay["b"].esize == 2 and CASES["b"].num_codes == 32768
    assert shards["c"] == [1, 1, 0] and lay["c"].esize == 4 and CASES["c"].num_codes == 32769
    assert shards["d"] == [2] * 5 + [1] * 3
    assert shards["e"] == [1] * 8
    assert shards["f"] == [1, 1, 1, 1, 0]
    assert shards["g"].count(0) == 13
    h = CASES["h"]
    assert _xch_grid(max(shards["h"]) * h.cpi) == 1 and max(shards["h"]) * h.gpi > 256 and lay["h"].esize == 4 and h.gpi > h.cpi
    assert max(shards["i"]) * CASES["i"].cpi > 2048 * 256 and CASES["i"].world == 1
    for n in ("j", "l"):
        assert CASES[n].batch * CASES[n].cpi > 2048 * 256 and lay[n].esize == 4
    assert len(set(shards["j"])) == 1 and len(set(shards["l"])) == 2
    assert len(set(shards["k"])) == 2 and (CASES["k"].cpi, CASES["k"].gpi) == (1024, 256)
    for n in NAMES:                                             # the forced codes really travel
        i = _inputs(n)
        assert all(c.max() == CASES[n].num_codes - 1 for c in i.codes if c.size)
        assert all(m is None for m, (s, z) in zip(i.loss, i.shards) if z == 0)


def test_rank_of_image_agrees_with_shard_slice():
    for world in range(1, 17):
        for B in range(1, 65):
            b_max = 0
            for r in range(world):
                s, e = shard_slice(B, r, world)
                assert ref.shard(B, r, world) == (s, e - s)
                b_max = max(b_max, e - s)
                for img in range(s, e):
                    assert ref.rank_of_image(img, B, world) == r, (world, B, img)
            assert b_max == ref.b_max_of(B, world)


def _torch_shard(inp, r):
    """rank r's arguments of _pack_torch, as CodeExchange.start makes them for CPU tensors"""
    c = torch.from_numpy(inp.codes[r].copy())
    g = torch.from_numpy(inp.grain[r].copy()) if inp.case.gpi else None
    if inp.loss[r] is None:
        return c, g, torch.zeros((), dtype=torch.float64), 0.0
    return c, g, torch.tensor([inp.loss[r]], dtype=torch.float32).reshape(-1)[0].double() * inp.numel[r], inp.numel[r]


@pytest.mark.parametrize("name", NAMES)
def test_pack_torch_is_the_reference_byte_for_byte(name):
    inp = _inputs(name)
    for r in range(inp.case.world):
        c, g, lsum, numel = _torch_shard(inp, r)
        got = _pack_torch(c, g, lsum, numel, inp.case.num_codes, inp.b_max).numpy()
        assert got.dtype == np.uint8 and got.shape == (inp.L.nbytes,)
        assert np.array_equal(got, inp.bufs[r]), (name, r, np.flatnonzero(got != inp.bufs[r])[:8])


@pytest.mark.parametrize("name", NAMES)
def test_unpack_torch_of_the_reference_buffers(name):
    inp = _inputs(name)
    W, B, cpi, gpi, K = inp.case
    codes, grain, mean = _unpack_torch(torch.from_numpy(np.concatenate(inp.bufs)), W, B, (cpi,), (gpi,) if gpi else None, K)
    assert codes.dtype == torch.int64 and np.array_equal(codes.numpy(), inp.g_codes)
    assert (grain is None) if gpi == 0 else (grain.dtype == torch.int64 and np.array_equal(grain.numpy(), inp.g_grain))
    assert mean.dtype == torch.float32 and _bits(mean.numpy()) == _bits(inp.mean), (float(mean), float(inp.mean))


def test_torch_pack_without_elements_sends_no_loss():
    """an empty shard's loss (the mean of nothing: NaN) stays out of the pair, so the global mean is the other ranks'"""
    inp = _inputs("c")
    empty = inp.case.world - 1
    c, g, _, _ = _torch_shard(inp, empty)
    got = _pack_torch(c, g, torch.tensor(float("nan"), dtype=torch.float64), 0.0, inp.case.num_codes, inp.b_max).numpy()
    assert np.array_equal(got, inp.bufs[empty])
    assert np.array_equal(ref.pack(inp.codes[empty], inp.grain[empty], np.float32("nan"), 0.0, inp.b_max, inp.case.num_codes), inp.bufs[empty])
    assert np.isfinite(inp.mean)


def test_without_any_loss_the_mean_is_nan_in_both():
    inp = _inputs("b", with_loss=False)
    W, B, cpi, gpi, K = inp.case
    assert np.isnan(inp.mean)
    assert torch.isnan(_unpack_torch(torch.from_numpy(np.concatenate(inp.bufs)), W, B, (cpi,), (gpi,), K)[2])


# ---- GPU: one process plays every rank ----------------------------------------------------------------------------------------

Run = collections.namedtuple("Run", "wire guard codes codes_guard grain grain_guard mean mean_guard")


def _run(inp, dev, packed=None, want_mean=True, use_grain=True, stale_loss=False):
    """Pack every rank into its slice of one buffer (or upload `packed`), unpack, synchronise once, bring everything back.
    use_grain=False: the same codes at grain_per_image 0 with null grain pointers.  stale_loss: the empty ranks pass a loss
    pointer (to a NaN) with numel 0."""
    W, B, cpi, gpi, K = inp.case
    gpi = gpi if use_grain else 0
    nb = ref.layout(cpi, gpi, inp.b_max, K).nbytes
    assert _lib.checked.dvq_exchange_bytes(cpi, gpi, inp.b_max, K) == nb
    gathered = torch.full((W * nb + GUARD_BYTES,), FILL, dtype=torch.uint8, device=dev)
    assert gathered.data_ptr() % 256 == 0 and nb % 8 == 0
    out_c = torch.full((B * cpi + GUARD,), SENT, dtype=torch.int64, device=dev)
    out_g = torch.full((B * gpi + GUARD,), SENT, dtype=torch.int64, device=dev) if gpi else None
    out_m = torch.full((1 + GUARD,), SENT_F, dtype=torch.float32, device=dev)
    nan = torch.full((1,), float("nan"), dtype=torch.float32, device=dev)
    keep = []
    with _lib.on_device(dev):
        st = _lib.stream_ptr(dev)
        if packed is not None:
            gathered[:W * nb] = torch.from_numpy(np.ascontiguousarray(packed)).to(dev)
        else:
            for r, (_, b_local) in enumerate(inp.shards):
                c = torch.from_numpy(inp.codes[r].copy()).to(dev) if b_local else None
                g = torch.from_numpy(inp.grain[r].copy()).to(dev) if (b_local and gpi) else None
                m = torch.tensor([inp.loss[r]], dtype=torch.float32, device=dev) if inp.loss[r] is not None else None
                if m is None and b_local == 0 and stale_loss:
                    m = nan
                keep += [c, g, m]
                _lib.checked.dvq_exchange_pack(_lib.ptr(c), _lib.ptr(g), _lib.ptr(m), inp.numel[r], b_local, inp.b_max, cpi, gpi, K,
                                               gathered.data_ptr() + r * nb, st)
        _lib.checked.dvq_exchange_unpack(gathered.data_ptr(), W, B, cpi, gpi, K, out_c.data_ptr(), _lib.ptr(out_g),
                                         out_m.data_ptr() if want_mean else 0, st)
        torch.cuda.synchronize(dev)
    wire, oc, om = gathered.cpu().numpy(), out_c.cpu().numpy(), out_m.cpu().numpy()
    og = out_g.cpu().numpy() if gpi else None
    return Run(wire[:W * nb], wire[W * nb:], oc[:B * cpi].reshape(B, cpi), oc[B * cpi:],
               og[:B * gpi].reshape(B, gpi) if gpi else None, og[B * gpi:] if gpi else None, om[:1], om[1:])


def _check_outputs(inp, run, mean=True, grain=True):
    assert np.array_equal(run.codes, inp.g_codes)
    if inp.case.gpi and grain:
        assert np.array_equal(run.grain, inp.g_grain)
        assert (run.grain_guard == SENT).all()
    assert (run.guard == FILL).all() and (run.codes_guard == SENT).all() and (run.mean_guard == np.float32(SENT_F)).all()
    if mean:
        assert _bits(run.mean) == _bits(inp.mean), (float(run.mean[0]), float(inp.mean))


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_kernels_pack_the_reference_bytes_and_unpack_the_global_batch(dev, name):
    inp = _inputs(name)
    run = _run(inp, dev)
    nb = inp.L.nbytes
    for r in range(inp.case.world):
        got = run.wire[r * nb:(r + 1) * nb]
        assert np.array_equal(got, inp.bufs[r]), (name, r, np.flatnonzero(got != inp.bufs[r])[:8], inp.L)
    _check_outputs(inp, run)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CROSS)
def test_kernel_pack_then_torch_unpack(dev, name):
    inp = _inputs(name)
    W, B, cpi, gpi, K = inp.case
    run = _run(inp, dev)
    codes, grain, mean = _unpack_torch(torch.from_numpy(run.wire.copy()), W, B, (cpi,), (gpi,), K)
    assert np.array_equal(codes.numpy(), inp.g_codes) and np.array_equal(grain.numpy(), inp.g_grain)
    assert _bits(mean.numpy()) == _bits(inp.mean)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CROSS)
def test_reference_pack_then_kernel_unpack(dev, name):
    inp = _inputs(name)
    _check_outputs(inp, _run(inp, dev, packed=np.concatenate(inp.bufs)))


@pytest.mark.gpu
def test_null_grain_at_grain_per_image_zero(dev):
    """case e's codes without a grain map: both kernels take null grain pointers, the layout has no grain section"""
    inp = _inputs("e")
    W, B, cpi, _, K = inp.case
    run = _run(inp, dev, use_grain=False)
    bufs = [ref.pack(inp.codes[r], None, inp.loss[r], inp.numel[r], inp.b_max, K) for r in range(W)]
    assert np.array_equal(run.wire, np.concatenate(bufs))
    assert run.grain is None
    _check_outputs(inp, run, grain=False)


@pytest.mark.gpu
def test_null_mean(dev):
    inp = _inputs("d")
    run = _run(inp, dev, want_mean=False)
    _check_outputs(inp, run, mean=False)
    assert run.mean[0] == np.float32(SENT_F)


@pytest.mark.gpu
def test_no_rank_has_a_loss(dev):
    inp = _inputs("b", with_loss=False)
    run = _run(inp, dev)
    assert np.array_equal(run.wire, np.concatenate(inp.bufs))
    _check_outputs(inp, run, mean=False)
    assert np.isnan(inp.mean) and np.isnan(run.mean[0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("c", "g"))
def test_an_empty_rank_with_a_stale_loss_pointer(dev, name):
    """numel == 0: the pair is (0, 0) whatever the loss pointer holds (here a NaN, the mean of nothing)"""
    inp = _inputs(name)
    run = _run(inp, dev, stale_loss=True)
    assert np.array_equal(run.wire, np.concatenate(inp.bufs))
    _check_outputs(inp, run)


@pytest.mark.gpu
def test_null_pointers_are_an_empty_shard_s_alone(dev):
    """null codes / grain with images to pack, and a gathered buffer off the 8-byte grid, are refused before any launch"""
    buf = torch.zeros(256, dtype=torch.uint8, device=dev)
    one = torch.zeros(8, dtype=torch.int64, device=dev)
    p, q, st = buf.data_ptr(), one.data_ptr(), _lib.stream_ptr(dev)
    with pytest.raises(_lib.DvqError, match="null pointer"):
        _lib.checked.dvq_exchange_pack(0, q, 0, 0.0, 1, 1, 1, 1, 10, p, st)
    with pytest.raises(_lib.DvqError, match="null grain"):
        _lib.checked.dvq_exchange_pack(q, 0, 0, 0.0, 1, 1, 1, 1, 10, p, st)
    with pytest.raises(_lib.DvqError, match="8-byte aligned"):
        _lib.checked.dvq_exchange_unpack(p + 4, 1, 1, 1, 0, 10, q, 0, 0, st)
    torch.cuda.synchronize(dev)


# ---- GPU: three rank processes on the one device, through CodeExchange ----------------------------------------------------------

XW, XK, XC, XG = 3, 40000, (3, 5), (2, 2)
XBATCHES = (7, 2)                                               # 2 images on 3 ranks: rank 2 holds none


def _rank_main(rank, port):
    """what one of the three rank processes runs (started by the test below as a fresh interpreter)"""
    import datetime
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", rank=rank, world_size=XW, timeout=datetime.timedelta(seconds=60))   # before the GPU is touched
    try:
        from dynamicvectorquantization_amd.encode import CodeExchange
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        cpi, gpi = XC[0] * XC[1], XG[0] * XG[1]
        for B in XBATCHES:
            inp = make_inputs((XW, B, cpi, gpi, XK), 7000 + B)                 # every rank's inputs, from the seed
            b_local = inp.shards[rank][1]
            codes = torch.from_numpy(inp.codes[rank].copy()).reshape((b_local,) + XC).to(dev)
            grain = torch.from_numpy(inp.grain[rank].copy()).reshape((b_local,) + XG).to(dev)
            loss = torch.tensor([inp.loss[rank], 0.25], dtype=torch.float32, device=dev) if b_local else None
            assert (codes.data_ptr() == 0) == (b_local == 0)
            xch = CodeExchange(codes, grain, XK, B, numel_per_image=inp.npi)
            assert xch.on_gpu and xch.world == XW and xch.b_local == b_local and xch.nbytes == inp.L.nbytes
            for _ in range(2):                                                 # the second start meets the first one's bytes
                xch.start(codes, grain, loss)
                g_codes, g_grain, g_mean = xch.finish()
                torch.cuda.synchronize(dev)
                assert np.array_equal(xch.gathered.cpu().numpy(), np.concatenate(inp.bufs)), "wire bytes, B = %d" % B
                assert g_codes.shape == (B,) + XC and np.array_equal(g_codes.cpu().numpy().reshape(B, cpi), inp.g_codes), "codes, B = %d" % B
                assert g_grain.shape == (B,) + XG and np.array_equal(g_grain.cpu().numpy().reshape(B, gpi), inp.g_grain), "grain, B = %d" % B
                assert _bits(g_mean.cpu().numpy()) == _bits(inp.mean), "mean, B = %d: %r vs %r" % (B, float(g_mean), float(inp.mean))
        print("XCH_RANK_OK %d" % rank, flush=True)
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_code_exchange_three_ranks_one_device(dev):
    """CodeExchange on CUDA tensors at world 3, B = 7 (3 + 2 + 2) and B = 2 (1 + 1 + 0), num_codes = 40000: the wire bytes of every
    rank, the global tensors and the bits of the mean against inputs regenerated from the seed.  The parent polls the three
    children: the first non-zero exit, or 180 s, ends them all, so a failing rank cannot leave the others in the collective."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    code = "import sys; sys.path.insert(0, %r); from tests.test_exchange_shapes import _rank_main; _rank_main(int(sys.argv[1]), %d)" % (ROOT, port)
    env = dict(os.environ)
    env.pop("RANK", None)
    t0 = time.time()
    procs = [subprocess.Popen([sys.executable, "-c", code, str(r)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(XW)]
    deadline, why = t0 + 180.0, None
    while True:
        rcs = [p.poll() for p in procs]
        bad = [(r, rc) for r, rc in enumerate(rcs) if rc not in (None, 0)]
        if bad:
            why = "rank %d exited with code %d" % bad[0]
        elif time.time() > deadline:
            why = "no end after 180 s"
        if why is not None or all(rc == 0 for rc in rcs):
            break
        time.sleep(0.05)
    for p in procs:                                             # the processes started above, nothing by pattern
        if p.poll() is None:
            p.terminate()
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=10)[0])
        except subprocess.TimeoutExpired:
            p.kill()
            outs.append(p.communicate()[0])
    print("three rank processes on one device: %.1f s" % (time.time() - t0))
    assert why is None, (why, [o[-3000:] for o in outs])
    for r, o in enumerate(outs):
        assert "XCH_RANK_OK %d" % r in o, o[-3000:]
