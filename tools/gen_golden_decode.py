"""Golden data of the decode head, from the reference's own modules (CPU; needs a checkout of the reference, imported through
oracle.refimport; the tests read only the .npz files this writes).

  decode_head_dual.npz (+ _c0.._c3 parts)   the reference's Dualformer.decode_to_img chain (dqtransformer_uncond_entropy.py:174-178:
                        permuter.forward_back -> get_code_emb_with_depth -> .permute -> DualGrainVQModel.decode) with the quantizer
                        and the DecoderPositional.Decoder of configs/stage1/dqvae-entropy-dual-r05_imagenet.yml, a seeded
                        post_quant_conv and synth.codebook_trained, on the region-first token streams of image 0 of
                        permuter_reference_selftest.npz.  The input of decoder.conv_in is captured with a forward pre-hook that
                        aborts the trunk.  Stored: codes, the two position tables as the reference computed them, the captured
                        h_in, the decoder's position parameters, seeds and CRCs of the regenerated parameters.  The three
                        [256, 32, 32] float32 arrays are cut into four channel slabs so that no file exceeds 1 MiB.
  decode_head_fourier.npz   position_type "fourier": VectorQuantize2 with a 33-row codebook (padding row used), C = 16, 8 x 8
  decode_head_toy.npz       position_type "learned" (an embedding forward never applies): VectorQuantizer2 with 16 rows, C = 64

    python tools/gen_golden_decode.py
"""
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refimport  # noqa: E402
from dynamicvectorquantization_amd import synth  # noqa: E402
from tests import _decode_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
YAML = "configs/stage1/dqvae-entropy-dual-r05_imagenet.yml"


class _Captured(Exception):
    pass


def _capture_conv_in(decoder, run):
    cap = {}

    def hook(module, args):
        cap["h_in"] = args[0].detach().clone()
        raise _Captured()

    h = decoder.conv_in.register_forward_pre_hook(hook)
    try:
        run()
    except _Captured:
        pass
    finally:
        h.remove()
    return cap["h_in"]


def _position_tables(decoder, C, H, W):
    """the two biases as the reference's modules compute them on CPU, in application order"""
    pt = decoder.position_type
    first = second = None
    if pt == "fourier":
        first = decoder.position_bias.lff(decoder.position_bias.coord)
    elif pt == "fourier+learned":
        first = decoder.position_bias_fourier.lff(decoder.position_bias_fourier.coord)
        second = decoder.position_bias_learned(torch.zeros(1, C, H, W))
    return [None if t is None else t[0].numpy().copy() for t in (first, second)]


def _position_params(decoder):
    return {"param/" + k: v.numpy().copy() for k, v in decoder.state_dict().items() if k.startswith("position_bias")}


def _meta(**kw):
    return np.array(json.dumps(dict(torch=torch.__version__, numpy=np.__version__, threads=torch.get_num_threads(),
                                    reference="Corleone-Huang/DynamicVectorQuantization, CPU", **kw)))


def gen_dual():
    refimport.setup()
    tv = sys.modules["torchvision.transforms"]
    tv.Compose = lambda ts: None
    tv.ToPILImage = lambda *a, **k: None
    tv.ToTensor = lambda *a, **k: None
    import yaml
    from utils.utils import instantiate_from_config
    from models.stage1_dynamic.dqvae_dual_entropy import DualGrainVQModel
    from models.stage2_dynamic.dqtransformer_uncond_entropy import Dualformer
    from modules.dynamic_modules.permuter import DualGrainSeperatePermuter
    cfg = yaml.safe_load(open(os.path.join(refimport.REF, YAML)))["model"]["params"]
    torch.manual_seed(20260401)
    torch.set_grad_enabled(False)
    quantize = instantiate_from_config(cfg["vqconfig"]).eval()
    decoder = instantiate_from_config(cfg["decoderconfig"]).eval()
    K, D, C = 1024, cfg["quant_after_dim"], cfg["quant_before_dim"]
    E = synth.codebook_trained(K, D)
    quantize.codebook.weight.data[:-1].copy_(torch.from_numpy(E))
    conv = torch.nn.Conv2d(D, C, 1).eval()
    seeds = dict(conv_w=9701, conv_b=9702)
    cw = synth.normal(seeds["conv_w"], (C, D, 1, 1), 0.0, 1.0 / 16.0)
    cb = synth.normal(seeds["conv_b"], (C,), 0.0, 0.1)
    conv.weight.data.copy_(torch.from_numpy(cw))
    conv.bias.data.copy_(torch.from_numpy(cb))
    fs = types.SimpleNamespace(quantize=quantize, post_quant_conv=conv, decoder=decoder)
    fs.get_code_emb_with_depth = lambda code: DualGrainVQModel.get_code_emb_with_depth(fs, code)
    fs.decode = lambda quant, grain_indices=None: DualGrainVQModel.decode(fs, quant, grain_indices)
    model = types.SimpleNamespace(first_stage_model=fs, permuter=DualGrainSeperatePermuter(
        coarse_hw=16, fine_hw=32, content_pad_code=1024, content_eos_code=1025, coarse_position_pad_code=256,
        coarse_position_eos_code=257, fine_position_pad_code=1024, fine_position_eos_code=1025, fine_position_order="region-first"))
    p = np.load(os.path.join(OUT, "permuter_reference_selftest.npz"))
    streams = [torch.from_numpy(p["region_" + k][:1].astype(np.int64))
               for k in ("coarse_content", "fine_content", "coarse_position", "fine_position")]
    h_in = _capture_conv_in(decoder, lambda: Dualformer.decode_to_img(model, *streams)).numpy()
    codes = model.permuter.forward_back(*streams).numpy()
    assert np.array_equal(codes, p["indices"][:1].astype(np.int64)), "forward_back does not reproduce the fixture's code map"
    F, L = _position_tables(decoder, C, 32, 32)
    # the stored tensors satisfy the bound the tests assert (tests/test_decode.py: test_restatement_matches_golden)
    full = quantize.codebook.weight.data.numpy()
    T64, M = R.table64(full, cw, cb), R.magnitude(full, cw, cb)
    err = np.abs(h_in.astype(np.float64) - R.head(T64.astype(np.float32), F, L, codes))
    print("dual: conv error / M max %.3g" % float((np.abs(h_in.astype(np.float64) - R.head(T64.astype(np.float32), F, L, codes))
                                                    / R.gather_nchw(M, codes)).max()),
          "bound ok", bool((err <= R.bound(M, T64, F, L, codes, 1e-5)).all()))
    meta = _meta(yaml=YAML, seeds=seeds, torch_seed=20260401, chain="Dualformer.decode_to_img (dqtransformer_uncond_entropy.py:174-178)",
                 streams="tests/golden/permuter_reference_selftest.npz region_* of image 0")
    nparts = 4
    np.savez_compressed(os.path.join(OUT, "decode_head_dual.npz"), meta=meta, parts=np.array(nparts), codes=codes.astype(np.int16),
                        conv_w_crc=np.uint32(R.crc(cw)), conv_b_crc=np.uint32(R.crc(cb)), cb_crc=np.uint32(R.crc(E)),
                        pos_first_crc=np.uint32(R.crc(F)), pos_second_crc=np.uint32(R.crc(L)), h_in_crc=np.uint32(R.crc(h_in)),
                        position_type=np.array(decoder.position_type), **_position_params(decoder))
    step = C // nparts
    for i in range(nparts):
        s = slice(i * step, (i + 1) * step)
        out = os.path.join(OUT, "decode_head_dual_c%d.npz" % i)
        np.savez_compressed(out, pos_first=F[s], pos_second=L[s], h_in=h_in[:, s])
        print("wrote", out, "%.1f KiB" % (os.path.getsize(out) / 1024))


def gen_small(name, position_type, vq_kind, rows_arg, D, C, hw, seed):
    refimport.setup()
    from modules.dynamic_modules.DecoderPositional import Decoder
    VQ2, VQGAN = refimport.quantizers()
    torch.manual_seed(seed)
    torch.set_grad_enabled(False)
    if vq_kind == "VectorQuantize2":
        quantize = VQ2(codebook_size=rows_arg, codebook_dim=D).eval()
        weight = quantize.codebook.weight
    else:
        quantize = VQGAN(rows_arg, D, beta=0.25).eval()
        weight = quantize.embedding.weight
    rows = weight.shape[0]
    E = synth.normal(seed + 1, (rows, D), 0.0, 1.0)
    weight.data.copy_(torch.from_numpy(E))
    conv = torch.nn.Conv2d(D, C, 1).eval()
    cw = synth.normal(seed + 2, (C, D, 1, 1), 0.0, 1.0 / 16.0)
    cb = synth.normal(seed + 3, (C,), 0.0, 0.1)
    conv.weight.data.copy_(torch.from_numpy(cw))
    conv.bias.data.copy_(torch.from_numpy(cb))
    decoder = Decoder(ch=32, in_ch=C, out_ch=3, ch_mult=(1,), num_res_blocks=1, resolution=hw, attn_resolutions=[],
                      latent_size=hw, window_size=2, position_type=position_type).eval()
    codes = synth.randint(seed + 4, (2, hw, hw), rows).astype(np.int64)
    codes[0, 0, 0], codes[1, -1, -1] = rows - 1, 0
    quant = quantize.get_codebook_entry(torch.from_numpy(codes))          # [B, H, W, D], as get_code_emb_with_depth returns it
    h_in = _capture_conv_in(decoder, lambda: decoder(conv(quant.permute(0, 3, 1, 2)), None)).numpy()
    F, L = _position_tables(decoder, C, hw, hw)
    arrays = dict(codes=codes.astype(np.int16), h_in=h_in, cb_crc=np.uint32(R.crc(E)), conv_w_crc=np.uint32(R.crc(cw)),
                  conv_b_crc=np.uint32(R.crc(cb)), position_type=np.array(position_type), quantizer=np.array(vq_kind),
                  rows=np.array(rows), D=np.array(D), C=np.array(C), **_position_params(decoder))
    if F is not None:
        arrays["pos_first"] = F
    if L is not None:
        arrays["pos_second"] = L
    out = os.path.join(OUT, name + ".npz")
    np.savez_compressed(out, meta=_meta(seeds=dict(torch=seed, codebook=seed + 1, conv_w=seed + 2, conv_b=seed + 3, codes=seed + 4),
                                        chain="get_codebook_entry -> .permute(0, 3, 1, 2) -> post_quant_conv -> "
                                              "DecoderPositional.Decoder.forward up to conv_in"), **arrays)
    print("wrote", out, "%.1f KiB" % (os.path.getsize(out) / 1024))


def main():
    gen_dual()
    gen_small("decode_head_fourier", "fourier", "VectorQuantize2", 32, 32, 16, 8, 9720)
    gen_small("decode_head_toy", "learned", "VectorQuantizer2", 16, 32, 64, 8, 9730)


if __name__ == "__main__":
    main()
