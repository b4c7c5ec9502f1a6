"""The wire format of the image-parallel code exchange, stated on its own in numpy (include/dvq.h, "Wire format of the
image-parallel exchange").  Nothing here imports the package or shares a line with it: tests/test_exchange_shapes.py holds the
kernels of csrc/exchange.hip and the torch-op path of encode.all_gather_codes against this file.

One rank's buffer, `nbytes` long:

    [0, b_max cpi esize)             the rank's codes, image after image, as little-endian int16 (num_codes <= 32768) or int32;
                                     the images b_local .. b_max - 1 that the rank does not hold are zeros
    [.., off_grain)                  zeros up to the next multiple of 8
    [off_grain, off_grain + b_max gpi)  grain indices as int8, padded with zero images the same way
    [.., off_pair)                   zeros up to the next multiple of 8
    [off_pair, off_pair + 16)        (float64(float32 local mean) * numel, numel) as two float64; (0, 0) without a loss or with
                                     numel == 0

Rank r of `world` holds the images [r base + min(r, extra), ...) of global_batch = world base + extra, base + 1 of them where
r < extra and base otherwise; b_max = ceil(global_batch / world).  The global mean is the float64 sum over the ranks, in rank
order, of the first and of the second members of the pairs, divided in float64 and rounded once to float32."""
import collections

import numpy as np

Layout = collections.namedtuple("Layout", "esize off_grain off_pair nbytes")


def _up8(n):
    return -(-n // 8) * 8


def layout(cpi, gpi, b_max, num_codes):
    esize = 2 if num_codes <= 32768 else 4
    off_grain = _up8(b_max * cpi * esize)
    off_pair = off_grain + _up8(b_max * gpi)
    return Layout(esize, off_grain, off_pair, off_pair + 16)


def shard(global_batch, r, world):
    """(first image, number of images) of rank r"""
    base, extra = global_batch // world, global_batch % world
    return (r * (base + 1), base + 1) if r < extra else (extra * (base + 1) + (r - extra) * base, base)


def rank_of_image(img, global_batch, world):
    """the rank whose shard holds image `img`: the inverse of `shard`, in closed form"""
    base, extra = global_batch // world, global_batch % world
    split = extra * (base + 1)
    if img < split:
        return img // (base + 1)
    return extra + (img - split) // base          # img >= split implies base > 0: split == global_batch where base == 0


def b_max_of(global_batch, world):
    return -(-global_batch // world)


def pack(codes_local, grain_local, loss_mean, numel, b_max, num_codes):
    """codes_local [b_local, cpi] integers, grain_local [b_local, gpi] integers or None, loss_mean a float32 or None"""
    codes_local = np.asarray(codes_local)
    b_local, cpi = codes_local.shape
    gpi = 0 if grain_local is None else np.asarray(grain_local).shape[1]
    L = layout(cpi, gpi, b_max, num_codes)
    buf = np.zeros(L.nbytes, dtype=np.uint8)
    wire = codes_local.astype("<i2" if L.esize == 2 else "<i4").reshape(-1)
    buf[:wire.size * L.esize] = wire.view(np.uint8)
    if gpi:
        g = np.asarray(grain_local).astype(np.int8).reshape(-1)
        buf[L.off_grain:L.off_grain + g.size] = g.view(np.uint8)
    if loss_mean is not None and numel != 0:
        pair = np.array([np.float64(np.float32(loss_mean)) * np.float64(numel), np.float64(numel)], dtype="<f8")
        buf[L.off_pair:] = pair.view(np.uint8)
    return buf


def unpack(gathered, world, global_batch, cpi, gpi, num_codes):
    """gathered uint8 [world * nbytes] -> (codes int64 [global_batch, cpi], grain int64 [global_batch, gpi] or None, mean float32)"""
    L = layout(cpi, gpi, b_max_of(global_batch, world), num_codes)
    rows = np.ascontiguousarray(np.asarray(gathered, dtype=np.uint8)).reshape(world, L.nbytes)
    codes = np.empty((global_batch, cpi), dtype=np.int64)
    grain = np.empty((global_batch, gpi), dtype=np.int64) if gpi else None
    for img in range(global_batch):
        r = rank_of_image(img, global_batch, world)
        j = img - shard(global_batch, r, world)[0]
        c = rows[r, j * cpi * L.esize:(j + 1) * cpi * L.esize].copy().view("<i2" if L.esize == 2 else "<i4")
        codes[img] = c
        if gpi:
            grain[img] = rows[r, L.off_grain + j * gpi:L.off_grain + (j + 1) * gpi].copy().view(np.int8)
    s, n = np.float64(0.0), np.float64(0.0)
    for r in range(world):
        pair = rows[r, L.off_pair:].copy().view("<f8")
        s, n = s + pair[0], n + pair[1]
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.float32(s / n)
    return codes, grain, mean
