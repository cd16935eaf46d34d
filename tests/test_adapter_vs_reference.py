"""CPU: the host orchestration of ``IPAdapterXL`` (rows a8-a10 of SURVEY.md section 8) against what the reference's
OWN ``IPAdapterXL`` class (ip_adapter/ip_adapter.py:249-340, imported verbatim through oracle/refshim.py) did with the
same inputs, stored in tests/golden/refpin_ipadapter.pt by oracle/gen_refpins.py: which processors ``set_ip_adapter``
installs where, ``get_image_embeds`` (HarmonyAttention fused into the CLIP embedding, zero-image uncond branch), and
what ``generate`` hands to the pipeline (tiling, text || image token order, pooled embeddings, seed -> generator, kwargs
pass-through, scale).  Both runs get the same fake pipeline / CLIP objects (oracle/gen_refpins.py) and the same seeded
projection modules (here the oracle's, which are pinned to the reference's); nothing here needs a GPU because the HIP
modules are swapped for those CPU modules before any compute."""
import os

import torch

from oracle import modules as om
from oracle.detfill import det_fill
from oracle.gen_refpins import (GENERATOR_SEEDS, NCA, PLUS_CFG, PLUS_KWARGS, XL_KWARGS, FakeClip, FakeClipH, FakePipe,
                                FakeProc, adapter_modules, digest, fake_image)
from oracle.sdxl_unet import UNet2DConditionModel as OracleUNet
from oracle.sdxl_unet import tiny_config
from conftest import GOLDEN

HALF = torch.float16


def _golden():
    return torch.load(os.path.join(GOLDEN, "refpin_ipadapter.pt"))


def _check_call(kr, km, nca, atol):
    """the recorded pipeline kwargs of the reference (oracle.gen_refpins.record_call) against ours"""
    assert set(kr) == set(km)
    for k in kr:
        if torch.is_tensor(kr[k]):
            assert kr[k].shape == km[k].shape and torch.allclose(kr[k].float(), km[k].float(), atol=atol, rtol=atol), k
        elif kr[k] == NCA:                                  # test.py:38's stray kwarg travels through both
            assert k == "number_class_crossattention" and km[k] is nca
        elif isinstance(kr[k], tuple) and kr[k][:1] == ("generator",):
            assert isinstance(km[k], torch.Generator) and km[k].initial_seed() == kr[k][1], k
        else:
            assert kr[k] == km[k], k


def test_ipadapterxl_orchestration_matches_reference():
    g = _golden()["xl"]
    from imagharmony_amd.attention_processor import AttnProcessor2_0, IPAttnProcessor2_0
    from imagharmony_amd.ip_adapter import IPAdapterXL
    m_unet = det_fill(OracleUNet(tiny_config()), 5)
    m = IPAdapterXL(FakePipe(m_unet), None, None, "cpu", num_tokens=4, inference=True, dtype=HALF,
                    image_encoder=FakeClip(), clip_image_processor=FakeProc())
    assert m.clip_embeddings_dim == 128
    m.image_proj_model, m.number_class_crossattention = adapter_modules(om)
    out_m = m.generate(pil_image=fake_image(0), number_class_crossattention=m.number_class_crossattention, **XL_KWARGS)

    # set_ip_adapter: same processor kinds / shapes / skip flags under the same names
    rp, mp = g["processors"], m_unet.attn_processors
    assert list(rp) == list(mp) and len(rp) > 0
    for k, rec in rp.items():
        if rec[0] == "AttnProcessor2_0":
            assert isinstance(mp[k], AttnProcessor2_0), k
        else:
            kind, hidden, cross_dim, num_tokens, skip, k_shape, scale = rec
            assert kind == "IPAttnProcessor2_0" and isinstance(mp[k], IPAttnProcessor2_0), k
            assert (mp[k].hidden_size, mp[k].cross_attention_dim, mp[k].num_tokens, mp[k].skip) == \
                   (hidden, cross_dim, num_tokens, skip), k
            assert tuple(mp[k].to_k_ip.weight.shape) == k_shape
            assert mp[k].scale == scale == 0.6                                   # generate() -> set_scale
    # generate: identical encode_prompt calls and identical pipeline arguments
    assert g["encoded"] == m.pipe.encoded
    kr, km = g["call"], m.pipe.calls[-1]
    assert g["images"] == out_m == ["img"]
    assert kr["number_class_crossattention"] == NCA and kr["generator"] == ("generator", 42)
    _check_call(kr, km, m.number_class_crossattention, 2e-3)
    assert kr["prompt_embeds"].shape == (1, 77 + 4, 256)


def test_ipadapterplusxl_orchestration_matches_reference():
    """IPAdapterPlusXL (ip_adapter.py:389-478): Resampler over the penultimate hidden states of the image and of a
    zero image, then the same hand-over to the pipeline; multi-sample tiling (num_samples = 2)"""
    g = _golden()["plusxl"]
    from imagharmony_amd.ip_adapter import IPAdapterPlusXL
    m = IPAdapterPlusXL(FakePipe(det_fill(OracleUNet(tiny_config()), 5)), None, None, "cpu", num_tokens=16, dtype=HALF,
                        image_encoder=FakeClipH(), clip_image_processor=FakeProc())
    assert m.clip_hidden_size == 64
    m.image_proj_model = det_fill(om.Resampler(**PLUS_CFG), 9).to(HALF)
    out_m = m.generate(pil_image=fake_image(1), **PLUS_KWARGS)

    assert g["images"] == out_m == ["img", "img"] and g["encoded"] == m.pipe.encoded
    assert g["encoded"][0][0] == ("best quality, high quality",)                 # default prompts (ip_adapter.py:433-436)
    kr, km = g["call"], m.pipe.calls[-1]
    assert kr["generator"] == ("generator", 7)
    _check_call(kr, km, None, 3e-3)
    assert kr["prompt_embeds"].shape == (2, 77 + 16, 256)
    assert all(p.scale == 0.9 for p in m.pipe.unet.attn_processors.values() if hasattr(p, "to_k_ip"))


def test_get_generator_and_checkpoint_loading_match_reference(tmp_path):
    """get_generator (ip_adapter/utils.py:83-93) and load_ip_adapter of an ip_adapter.bin (ip_adapter.py:135-154): the
    checkpoint written from a donor adapter is the reference's tensor for tensor, and loading it leaves both adapters
    with the same weights in the projection, the HarmonyAttention module and the 70 -> (here 22) IP processors, keyed
    '<idx>.to_k_ip.weight' in attn_processors order (tensors compared through oracle.gen_refpins.digest)"""
    g = _golden()
    from imagharmony_amd.utils import get_generator
    for seed, want in zip(GENERATOR_SEEDS, g["get_generator"]):
        b = get_generator(seed, "cpu")
        if seed is None:
            assert want is None and b is None
        elif isinstance(seed, list):
            assert want == [x.initial_seed() for x in b] == seed
        else:
            assert want[0] == b.initial_seed() == seed and torch.equal(want[1], torch.randn(4, generator=b))

    # the checkpoint in the reference's own format, written from a donor adapter
    from imagharmony_amd.ip_adapter import IPAdapterXL
    donor_unet = det_fill(OracleUNet(tiny_config()), 5)
    IPAdapterXL(FakePipe(donor_unet), None, None, "cpu", num_tokens=4, inference=True, dtype=HALF, clip_embeddings_dim=128)
    for n, p in donor_unet.attn_processors.items():
        det_fill(p, 21, prefix=n)
    proj, ha = adapter_modules(om)
    layers = torch.nn.ModuleList(donor_unet.attn_processors.values())
    ckpt = {"image_proj": det_fill(proj, 31).state_dict(), "ip_adapter": layers.state_dict(),
            "composed_adapter": det_fill(ha, 33).state_dict()}
    assert list(ckpt) == list(g["checkpoint"])
    for grp in ckpt:
        assert digest(ckpt[grp]) == g["checkpoint"][grp], grp
    path = str(tmp_path / "ip_adapter.bin")
    torch.save(ckpt, path)
    assert sorted(layers.state_dict())[0].endswith(".to_k_ip.weight") and len(layers.state_dict()) == 2 * sum(
        hasattr(p, "to_k_ip") for p in donor_unet.attn_processors.values())

    from imagharmony_amd.modules import HarmonyAttention
    hm = HarmonyAttention(image_hidden_size=128, text_context_dim=256, inter_dim=512, cross_heads=8, reshape_blocks=8,
                          cross_value_dim=64, scale=1.0, fusion_method="cross_attention")
    m = IPAdapterXL(FakePipe(det_fill(OracleUNet(tiny_config()), 5)), None, path, "cpu", num_tokens=4, inference=True,
                    number_class_crossattention=hm, dtype=HALF, clip_embeddings_dim=128)      # loads in __init__ (ip_adapter.py:89)
    assert digest(m.image_proj_model.state_dict()) == g["loaded"]["image_proj"]
    assert digest(m.number_class_crossattention.state_dict()) == g["loaded"]["composed_adapter"]
    assert digest(torch.nn.ModuleList(m.pipe.unet.attn_processors.values()).state_dict()) == g["loaded"]["ip_adapter"]
