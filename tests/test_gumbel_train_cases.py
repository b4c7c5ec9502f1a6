"""GumbelQuantize's training step (csrc/vq_gumbel_backward.hip, quantize.gumbel_quantize), what holds without a GPU: the ABI of the
two new entry points, the float64 restatement of dL/dlogits against torch autograd, and the baseline the kernel's tolerance
stands on.  Rules and reference: tests/_gumbel_train_ref.py; cases: tests/_score_cases.GUMBEL_CASES.

The baseline.  ERR_REF = 2.4e-6 is the largest max |dl32 - dl64| / max |dl64| of the reference's own op sequence in float32 on the
CPU (torch autograd of gumbel-softmax-hard + einsum + KL with the kernel's logits as the leaf) over the table, for the mixes
(G ~ N(0, 1), g_kl = 0.35) and (no G, g_kl = 1); the kernel's bound on the GPU is 8 ERR_REF = 1.9e-5.  The test below measures the
baseline again, prints it per case and asserts that it stays within ERR_REF, so the constant cannot drift from what it stands for."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import _gumbel_train_ref as T
from tests import _score_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dvq_vq_gumbel_forward_train_f32", "dvq_vq_gumbel_backward_f32")


def test_the_symbols_are_declared_and_exported_and_the_version_stays():
    from dynamicvectorquantization_amd import _lib
    header = open(os.path.join(ROOT, "include", "dvq.h")).read()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name), name
        assert "DVQ_API int %s(" % name in header
        assert _lib._PROTOTYPES[name][0] is ctypes.c_int
    assert _lib.lib.dvq_version() == 2000
    assert set(_lib._TABLED_GUMBEL_TRAIN) == set(NEW)
    # the training forward is the assign's prototype with `logits` in front of the workspace; the backward takes 13 arguments
    assign, train = _lib._PROTOTYPES["dvq_vq_gumbel_assign_f32"][1], _lib._PROTOTYPES[NEW[0]][1]
    assert train == assign[:14] + [ctypes.c_void_p] + assign[14:]
    assert len(_lib._PROTOTYPES[NEW[1]][1]) == 13
    for fn in NEW:                                              # status calls like the rest: checked.* raises
        with pytest.raises(_lib.DvqError, match="null pointer"):
            getattr(_lib.checked, fn)(*([0] * len(_lib._PROTOTYPES[fn][1])))


def test_the_argument_rejections_hold():
    """tests/golden/abi_rejections_gumbel_train.json, replayed as tests/test_abi_rejections.py replays its table: in a child process
    that sees no GPU, so that a check a later edit loses shows as a wrong rc and never as a kernel on the fake pointers"""
    table = os.path.join(ROOT, "tests", "golden", "abi_rejections_gumbel_train.json")
    rows = json.load(open(table))
    assert {r["fn"] for r in rows} == set(NEW) and len(rows) >= 30
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    tool = os.path.join(ROOT, "tools", "gen_golden_abi_rejections.py")
    out = subprocess.run([sys.executable, tool, "--replay", table], env=env, check=True, capture_output=True, text=True, timeout=120).stdout
    got = json.loads(out)
    assert len(got) == len(rows)
    messages = {fn: set() for fn in NEW}
    for r, (rc, message) in zip(rows, got):
        assert r["rc"] in (-1, -2, -3), r
        assert (rc, message) == (r["rc"], r["message"]), (r["fn"], r["args"])
        messages[r["fn"]].add(message.split(": ", 1)[1])
    # the forward refuses what dvq_vq_gumbel_assign_f32 refuses, in its words
    number = lambda ms: {re.sub(r"-?\d+", "#", m) for m in ms}
    assign = {r["message"].split(": ", 1)[1] for r in json.load(open(os.path.join(ROOT, "tests", "golden", "abi_rejections.json")))
              if r["fn"] == "dvq_vq_gumbel_assign_f32"}
    assert len(assign) >= 9 and number(assign) <= number(messages[NEW[0]])
    back = messages[NEW[1]]
    for part in ("null pointer", "must be positive", "tau=0 must be finite and positive when u is given",
                 "kl_K=inf must be finite and positive when g_kl is given", "tensor too large", "misaligned pointer",
                 "dlogits may alias u only"):
        assert any(part in m for m in back), part


@pytest.mark.parametrize("name", ["w-C64-K1-q", "w-C64-K5-noq", "w-C128-K100-q", "kl-inf40", "kl-one", "kl-allinf", "kl-std30", "kl-klK1000.5"])
def test_the_restatement_is_the_float64_autograd_of_the_reference(name, oracle_mod):
    """dl64 against torch autograd in float64 with the same leaf, the reference's 1e-10 included: the two differ by that 1e-10
    alone (below 1e-9 of the largest entry); codes at -inf get exactly 0 from both; a token of all -inf is NaN in both"""
    c = C.G_BY_NAME[name]
    inp, tr = C.gumbel_inputs(c, oracle_mod), T.train_inputs(c, oracle_mod)
    for mix, with_u, g_kl in T.MIXES:
        want = tr[mix]
        # (the chain's own einsum forms u in float64 from G and E; the restatement was given fl32(u): compare on that u instead)
        u = tr["u32"].astype(np.float64) if with_u else None
        got = T.dl64(inp["l32"], tr["qrows"], u, g_kl, c.tau, inp["kl_K"])
        assert np.array_equal(got, want, equal_nan=True)
        chain = T.torch_chain(inp["l32"], tr["qrows"], inp["E"], tr["G"] if with_u else None, g_kl, c.tau, inp["kl_K"], torch_f64())
        exact_u = T.dl64(inp["l32"], tr["qrows"], tr["G"].astype(np.float64) @ inp["E"].astype(np.float64).T if with_u else None,
                         g_kl, c.tau, inp["kl_K"])
        err, same_nan = T.error(chain, exact_u, u, c.tau)
        assert same_nan and err <= 1e-9, (name, mix, err)
        if c.bias == "allinf":
            assert np.isnan(want).all()
        if c.bias in ("inf40", "one"):
            dead = ~np.isfinite(inp["b"])
            assert dead.any() and not want[:, dead].any() and not chain[:, dead].any()
        if c.K == 1 or c.bias == "one":
            assert not want.any()


def torch_f64():
    import torch
    return torch.float64


def test_the_float32_chain_of_the_reference_stays_within_err_ref(oracle_mod):
    """the baseline of the kernel's tolerance, measured again: per case and mix max |dl32 - dl64| / max |dl64|"""
    import torch
    worst = {}
    for c in C.GUMBEL_CASES:
        inp, tr = C.gumbel_inputs(c, oracle_mod), T.train_inputs(c, oracle_mod)
        for mix, with_u, g_kl in T.BASELINE_MIXES:
            G = tr["G"] if with_u else None
            want = T.dl64(inp["l32"], tr["qrows"], tr["G"].astype(np.float64) @ inp["E"].astype(np.float64).T if with_u else None,
                          g_kl, c.tau, inp["kl_K"])
            got = T.torch_chain(inp["l32"], tr["qrows"], inp["E"], G, g_kl, c.tau, inp["kl_K"], torch.float32)
            err, same_nan = T.error(got, want, tr["u32"] if with_u else None, c.tau)
            assert same_nan, (c.name, mix)
            print("%s %s: float32 chain %.3g" % (c.name, mix, err))
            if err > worst.get(mix, (0.0, ""))[0]:
                worst[mix] = (err, c.name)
            # where dl64 is identically zero the chain's own rounding of y (u - delta) shows against max |u| / tau: within the bound too
            assert err <= T.ERR_REF, (c.name, mix, err)
    print("largest:", worst)
    assert abs(8 * T.ERR_REF - T.BOUND) <= 1e-6


def test_the_float32_chain_on_the_multi_chunk_cases():
    """the same baseline for the cases that run the backward's code loop over several chunks (tests/_gumbel_train_ref.CHUNK_CASES):
    it stays within CHUNK_ERR_REF, and the bound the kernel is held to there, BOUND, is no wider than 8 x that"""
    import torch
    worst = (0.0, "")
    for c in T.CHUNK_CASES:
        inp = T.chunk_inputs(c)
        for mix, with_u, g_kl in T.MIXES:
            u = inp["u32"] if with_u else None
            got = T.torch_chain_u(inp["l32"], inp["qrows"], u, g_kl, c.tau, inp["kl_K"], torch.float32)
            err, same_nan = T.error(got, inp[mix], u, c.tau)
            print("%s %s: float32 chain %.3g" % (c.name, mix, err))
            assert same_nan and err <= T.CHUNK_ERR_REF, (c.name, mix, err)
            worst = max(worst, (err, c.name + " " + mix))
            if c.kind == "inf_lead":
                assert np.isnan(inp[mix][list(T.CHUNK_NAN_ROWS)]).all() and not inp[mix][:, inp["dead"]][8:].any()
    print("largest:", worst)
    assert T.BOUND <= 8 * T.CHUNK_ERR_REF
    # every case is several chunks of its form: 256 codes a chunk below 1024 workgroups of 32 tokens, 64 from there
    for c in T.CHUNK_CASES:
        chunk = 256 if (c.B * c.HW + 31) // 32 < 1024 else 64
        assert c.K > 2 * chunk and c.K % chunk != 0 and c.lead > chunk
    assert {(c.B * c.HW + 31) // 32 < 1024 for c in T.CHUNK_CASES} == {True, False}
