"""The permuter kernels (csrc/permute.hip) at every coarse grid form up to 32 x 32: a fraction of one chunk of 256 cells,
exactly one, one and a ragged second (17 x 17, 20 x 20), and four (32 x 32), where the running base and the rank table cross a
chunk edge.  Integer work: every stream is compared bit for bit with the numpy oracle (oracle/permuter.py)."""
import numpy as np
import pytest
import torch

from dynamicvectorquantization_amd import _lib
from oracle import permuter as P

GRIDS = (1, 2, 3, 5, 8, 15, 16, 17, 20, 31, 32)
ORDERS = ("region-first", "row-first")
KEYS = ["coarse_content", "fine_content", "coarse_position", "fine_position", "coarse_segment", "fine_segment"]
K = 1024                                                 # content codes 0 .. K - 1


def _codes(hc):
    """pad / eos codes above every content code and position of the grid (the defaults collide above 16 x 16)"""
    n = hc * hc
    return dict(content_pad=K, content_eos=K + 1, cpos_pad=n, cpos_eos=n + 1, fpos_pad=4 * n, fpos_eos=4 * n + 1)


def _permuter(hc, order="region-first"):
    from dynamicvectorquantization_amd.permuter import DualGrainSeperatePermuter
    c = _codes(hc)
    return DualGrainSeperatePermuter(coarse_hw=hc, fine_hw=2 * hc, content_pad_code=c["content_pad"],
                                     content_eos_code=c["content_eos"], coarse_position_pad_code=c["cpos_pad"],
                                     coarse_position_eos_code=c["cpos_eos"], fine_position_pad_code=c["fpos_pad"],
                                     fine_position_eos_code=c["fpos_eos"], fine_position_order=order)


def _batch(hc):
    """B = 6: grain maps at fine fractions 0.1, 0.5, 0.9, all coarse, all fine, fine in the last grid row only.  A coarse
    cell holds one code four times, as the encoder writes it (the round trip restores the input only then)."""
    g = np.random.default_rng(900 + hc)
    grain = np.stack([(g.random((hc, hc)) < f).astype(np.int64) for f in (0.1, 0.5, 0.9)] +
                     [np.zeros((hc, hc), np.int64), np.ones((hc, hc), np.int64), np.zeros((hc, hc), np.int64)])
    grain[5, -1, :] = 1
    fine = g.integers(0, K, (6, 2 * hc, 2 * hc))
    coarse = g.integers(0, K, (6, hc, hc)).repeat(2, axis=-1).repeat(2, axis=-2)
    idx = np.where(grain.repeat(2, axis=-1).repeat(2, axis=-2) == 1, fine, coarse)
    return idx, grain


def _oracle_forward(idx, grain, hc, order):
    return P.forward(idx, grain, coarse_hw=hc, fine_hw=2 * hc, order=order, **_codes(hc))


def test_oracle_serves_every_grid():
    """CPU: the oracle's own round trip at the grids the GPU tests compare against"""
    for hc in GRIDS:
        idx, grain = _batch(hc)
        c = _codes(hc)
        for order in ORDERS:
            o = _oracle_forward(idx, grain, hc, order)
            assert o["coarse_content"].shape[1] == hc * hc + 1 and o["fine_content"].shape[1] == 4 * hc * hc + 1
            back = P.forward_back(o["coarse_content"], o["fine_content"], o["coarse_position"], o["fine_position"],
                                  coarse_hw=hc, fine_hw=2 * hc, cpos_eos=c["cpos_eos"], fpos_eos=c["fpos_eos"])
            assert np.array_equal(back, idx)


@pytest.mark.gpu
@pytest.mark.parametrize("hc", GRIDS)
@pytest.mark.parametrize("order", ORDERS)
def test_forward_and_round_trip_at_every_grid_form(dev, hc, order):
    idx, grain = _batch(hc)
    c = _codes(hc)
    perm = _permuter(hc, order)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    want = _oracle_forward(idx, grain, hc, order)
    out = perm(t(idx), t(grain))
    for k in KEYS:
        assert out[k].dtype == torch.int64
        assert np.array_equal(out[k].cpu().numpy(), want[k]), (hc, order, k)
    back = perm.forward_back(out["coarse_content"], out["fine_content"], out["coarse_position"], out["fine_position"])
    assert np.array_equal(back.cpu().numpy(), idx)
    # max_len = max_lengths(): the same streams, then PAD.  This batch holds an all-coarse and an all-fine image, so the
    # oracle's streams already have the full lengths; three more columns show the tail
    Lc, Lf = perm.max_lengths()
    assert (Lc, Lf) == (hc * hc + 1, 4 * hc * hc + 1) == (want["coarse_content"].shape[1], want["fine_content"].shape[1])
    pads = {"coarse_content": c["content_pad"], "fine_content": c["content_pad"], "coarse_position": c["cpos_pad"],
            "fine_position": c["fpos_pad"], "coarse_segment": 0, "fine_segment": 1}
    for lens in ((Lc, Lf), (Lc + 3, Lf + 3)):
        got = perm(t(idx), t(grain), max_len=lens)
        for k in KEYS:
            a = got[k].cpu().numpy()
            L = want[k].shape[1]
            assert a.shape[1] == (lens[0] if k.startswith("coarse") else lens[1])
            assert np.array_equal(a[:, :L], want[k]) and (a[:, L:] == pads[k]).all(), (hc, order, k, lens)
        back = perm.forward_back(got["coarse_content"], got["fine_content"], got["coarse_position"], got["fine_position"])
        assert np.array_equal(back.cpu().numpy(), idx)
    # a batch without the two full images has shorter streams: max_lengths() pads them
    sub = [0, 1, 2, 5]
    want_sub = _oracle_forward(idx[sub], grain[sub], hc, order)
    got = perm(t(idx[sub]), t(grain[sub]), max_len=(Lc, Lf))
    for k in KEYS:
        a = got[k].cpu().numpy()
        L = want_sub[k].shape[1]
        assert np.array_equal(a[:, :L], want_sub[k]) and (a[:, L:] == pads[k]).all(), (hc, order, k)
    # too short: exactly the prefix (entries that do not fit are dropped, the EOS included)
    for lens in sorted({(1, 1), (max(Lc // 2, 1), max(Lf // 2, 1)), (max(Lc - 1, 1), max(Lf - 1, 1)), (Lc, 2), (1, Lf)}):
        got = perm(t(idx), t(grain), max_len=lens)
        for k in KEYS:
            L = lens[0] if k.startswith("coarse") else lens[1]
            assert np.array_equal(got[k].cpu().numpy(), want[k][:, :L]), (hc, order, k, lens)


def _without_out_of_range(content, position, eos, limit, pad):
    """the streams with the entries before the EOS whose position lies outside [0, limit) taken out (the kernel ignores
    them; the oracle, like the reference, would index out of bounds), the rest moved up and the tail padded"""
    content, position = np.array(content), np.array(position)
    for i in range(position.shape[0]):
        hits = np.flatnonzero(position[i] == eos)
        end = hits[0] if len(hits) else position.shape[1]
        keep = np.ones(position.shape[1], bool)
        keep[:end] = (position[i, :end] >= 0) & (position[i, :end] < limit)
        n = int(keep.sum())
        content[i] = np.concatenate([content[i][keep], np.full(len(keep) - n, pad)])
        position[i] = np.concatenate([position[i][keep], np.full(len(keep) - n, eos if len(hits) else limit)])
    return content, position


@pytest.mark.gpu
@pytest.mark.parametrize("hc", (17, 32))
def test_forward_back_semantics_off_the_default_grid(dev, hc):
    """hand-made streams: a later entry wins, entries after the EOS are ignored, positions outside the grid are ignored,
    no EOS in the coarse stream -> no upsample"""
    n, c = hc * hc, _codes(hc)
    ceos, feos = c["cpos_eos"], c["fpos_eos"]
    g = np.random.default_rng(40 + hc)
    Lc, Lf = n + 30, 4 * n + 30
    B = 5
    cp = np.full((B, Lc), c["cpos_pad"], np.int64)
    fp = np.full((B, Lf), c["fpos_pad"], np.int64)
    cc, fc = g.integers(1, K, (B, Lc)), g.integers(1, K, (B, Lf))
    # 0: every coarse cell, then the cells on both sides of 255 / 256 again (the later entry wins); fine positions with repeats
    cp[0, :n] = g.permutation(n)
    cp[0, n:n + 20] = np.arange(246, 266)
    cp[0, n + 20] = ceos
    fp[0, :600] = g.integers(0, 4 * n, 600)
    fp[0, 600] = feos
    # 1: entries after the EOS (valid positions, and a second EOS) are ignored
    cp[1, :40] = g.integers(0, n, 40)
    cp[1, 40] = ceos
    cp[1, 41:60] = g.integers(0, n, 19)
    cp[1, 60] = ceos
    fp[1, :50] = g.integers(0, 4 * n, 50)
    fp[1, 50] = feos
    fp[1, 51:200] = g.integers(0, 4 * n, 149)
    # 2: no coarse EOS: the coarse stream is not applied, the fine one is
    cp[2] = g.integers(0, n, Lc)
    fp[2, :300] = g.integers(0, 4 * n, 300)
    fp[2, 300] = feos
    # 3: no EOS in either stream, every column holds a position
    cp[3] = g.integers(0, n, Lc)
    fp[3] = g.integers(0, 4 * n, Lf)
    # 4: positions outside the grid before the EOS (the pad code, negative, far above), between valid ones
    cp[4, :12] = [5, c["cpos_pad"], -1, n, n + 7, 2 ** 40, 256 % n, 255, -2 ** 40, 5, n - 1, ceos]
    fp[4, :12] = [9, c["fpos_pad"], -3, 4 * n, 4 * n + 9, 2 ** 40, 1024 % (4 * n), 1023, -2 ** 40, 9, 4 * n - 1, feos]
    perm = _permuter(hc)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    got = perm.forward_back(t(cc), t(fc), t(cp), t(fp)).cpu().numpy()
    occ, ocp = _without_out_of_range(cc, cp, ceos, n, c["content_pad"])
    ofc, ofp = _without_out_of_range(fc, fp, feos, 4 * n, c["content_pad"])
    assert np.array_equal(occ[:4], cc[:4]) and np.array_equal(ofp[:4], fp[:4])      # rows 0-3 reach the oracle as they are
    want = P.forward_back(occ, ofc, ocp, ofp, coarse_hw=hc, fine_hw=2 * hc, cpos_eos=ceos, fpos_eos=feos)
    assert np.array_equal(got, want)
    assert (got[2] != 0).sum() <= 300 and (got[3] != 0).sum() <= Lf                 # no upsample without a coarse EOS
    assert (got[0] != 0).all()                                                       # every cell written


@pytest.mark.gpu
def test_grid_of_33_raises(dev):
    perm = _permuter(33)
    idx = torch.zeros(1, 66, 66, dtype=torch.long, device=dev)
    grain = torch.zeros(1, 33, 33, dtype=torch.long, device=dev)
    with pytest.raises(_lib.DvqError):
        perm(idx, grain)
    with pytest.raises(_lib.DvqError):
        perm(idx, grain, max_len=perm.max_lengths())
    seq = torch.zeros(1, 8, dtype=torch.long, device=dev)
    with pytest.raises(_lib.DvqError):
        perm.forward_back(seq, seq, seq, seq)
