"""GPU (-m gpu): the tuning build's diagnostic pointers reach every translation unit that reads them.  Pass 1 is compiled as one
unit per (D, resident seed table) and the resolver as another (csrc/dvq_pass1.h, csrc/vq_pass1_d*.hip, csrc/vq_resolve.hip);
device code is not relocatable, so each unit holds its own copy of g_dvq_tokdbg / g_dvq_stamps and dvq_tuning_buffers has to
set them all.  A copy left null would silently switch its kernels' diagnostics off: tools/bound_audit.py --production would then
audit a buffer of NaNs for that D and K."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUNE = os.path.join(ROOT, "dynamicvectorquantization_amd", "csrc", "libdvq_tuning.so")

# (N, K): 8322 tokens are past the 8192-token split form and leave a ragged last block: the plain (D = 64, 128) or cached
# (D = 256) form runs, with the resident seed table at K = 96 (3 code tiles) and without at K = 1056 (33 tiles, one more than
# the table holds).  130 tokens are a small batch: K = 96 leaves a slice fewer than the two tiles the split form asks for (the
# plain / cached form runs again), at K = 1056 the split form runs, 8 slices of at most 5 tiles.
SHAPES = [(8322, 96), (8322, 1056), (130, 96), (130, 1056)]

CHILD = r"""
import json, sys
import numpy as np
import torch
from dynamicvectorquantization_amd import _lib, synth
from dynamicvectorquantization_amd.quantize import _CodebookPrep, vq_assign

assert hasattr(_lib.lib, "dvq_tuning_buffers")
dev = torch.device("cuda:0")
for D in (64, 128, 256):
    for N, K in json.loads(sys.argv[1]):
        E = synth.codebook_trained(K, D)
        z = torch.from_numpy(synth.z_tokens(E, 1, 1, N, 7100 + D + K).reshape(1, D, N)).to(dev)
        Et = torch.from_numpy(E).to(dev)
        dbg = torch.full((N, 4), float("nan"), dtype=torch.float32, device=dev)
        # stamps: [workgroup][8] of the split form (at most 256 workgroups), the resolver's from row 4096 on (a workgroup per 32
        # record slots: 128 + at most one per queue shard for these N) -- 8192 rows are several times what either writes
        stamps = torch.zeros((8192, 8), dtype=torch.int64, device=dev)
        prep = _CodebookPrep()
        assert _lib.lib.dvq_tuning_buffers(stamps.data_ptr(), dbg.data_ptr()) == 0
        try:
            _, codes, _ = vq_assign(z, Et, prep, None, want_zq=False, want_loss=False, mode=_lib.MODE_FILTER_PASS1)
            torch.cuda.synchronize()
            d = dbg.cpu().numpy()
            p1_stamp = int(stamps[0, 0])
            _, codes_full, _ = vq_assign(z, Et, prep, None, want_zq=False, want_loss=False, mode=_lib.MODE_FILTER)
            torch.cuda.synchronize()
        finally:
            _lib.lib.dvq_tuning_buffers(0, 0)
        c = codes.cpu().numpy().reshape(-1)
        print(json.dumps({"D": D, "N": N, "K": K, "rows_written": int(np.isfinite(d).all(axis=1).sum()),
                          "codes_equal": bool(np.array_equal(d[:, 3].astype(np.int64), c)),
                          "pass1_stamp": p1_stamp, "resolver_stamp": int(stamps[4096, 0])}))
"""


def test_every_unit_copy_of_the_tuning_pointers_is_set(dev):
    """per D in {64, 128, 256} and SHAPES: the [N, 4] debug buffer, pre-filled with NaN, is written for every token by
    MODE_FILTER_PASS1 (finite latents: no token goes to the exact list) and its code column is the codes the call returned --
    the six pass-1 units; the split form's workgroup 0 and the resolver's workgroup 0 leave their first clock stamps -- the
    stamp pointer of the pass-1 units and of the resolver's.  A child process with DVQ_LIBRARY = libdvq_tuning.so."""
    if not os.path.exists(TUNE):
        pytest.skip("libdvq_tuning.so not built (make -C dynamicvectorquantization_amd/csrc tuning)")
    r = subprocess.run([sys.executable, "-c", CHILD, json.dumps(SHAPES)], cwd=ROOT,
                       env=dict(os.environ, DVQ_LIBRARY=TUNE), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    rows = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(rows) == 3 * len(SHAPES)
    for x in rows:
        assert x["rows_written"] == x["N"], x
        assert x["codes_equal"], x
        assert x["resolver_stamp"] != 0, x
        if (x["N"], x["K"]) == (130, 1056):                  # the split form: the only one of pass 1 that stamps
            assert x["pass1_stamp"] != 0, x
