"""CPU: LoRA's host side (imagharmony_amd.lora, include/imh_lora.h) -- the four key namings, the name tables against the SDXL manifest,
every refusal, the bookkeeping of the concatenated factors and strengths (against a LoRAState whose device side is a recorder), the
header / binding of the two new entries and their argument refusals (validation precedes the launch, so that runs without a device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tiny_cfg():
    from imagharmony_amd.unet import UNetConfig
    return UNetConfig(block_out_channels=(64, 128, 256), transformer_layers_per_block=(1, 1, 2), attention_head_dim=(1, 2, 4),
                      cross_attention_dim=256, addition_time_embed_dim=64, projection_class_embeddings_input_dim=128 + 6 * 64, sample_size=32)


def _tiny_unet():
    from imagharmony_amd.unet import UNet2DConditionModel
    u = UNet2DConditionModel(_tiny_cfg())
    with torch.no_grad():
        for p in u.parameters():
            p.zero_()
    return u


def _recorder(unet):
    from imagharmony_amd.lora import LoRAState

    class Rec(LoRAState):
        """the device side replaced: no weight check, no upload; apply() records the strengths it would have copied"""

        def __init__(self, u):
            super().__init__(u)
            self.calls = []

        def _check_weights(self, names):
            pass

        def _upload(self):
            pass

        def apply(self):
            self.calls.append(self._fill_g().copy())

    return Rec(unet)


def _manifest_weights():
    out = {}
    for line in open(os.path.join(ROOT, "tests", "golden", "sdxl_unet_manifest.txt")):
        name, shape = line.split()
        if name.endswith(".weight") and shape.count("x") in (1, 3):
            out[name[:-len(".weight")]] = tuple(int(s) for s in shape.split("x"))
    return out


# ---------------------------------------------------------------------------------------------------- parsing
def test_four_namings_parse_to_one_canonical_dict():
    from imagharmony_amd import lora
    cfg = _tiny_cfg()
    ref = None
    for naming in ("diffusers", "peft_old", "kohya", "sgm"):
        sd = lora.synthetic_adapter(cfg, rank=3, seed=11, naming=naming, alpha=1.5)
        canon, skipped = lora.parse_state_dict(sd, cfg)
        assert skipped == [] and len(canon) == len(lora.adaptable_modules(lora._meta_unet(cfg))) == len(sd) // 3
        if ref is None:
            ref = canon
            continue
        assert list(canon) == list(ref)
        for k in ref:
            assert torch.equal(canon[k][0], ref[k][0]) and torch.equal(canon[k][1], ref[k][1]) and canon[k][2] == ref[k][2] == 1.5
    # a conv pair keeps its 4-D shapes; the prefix "unet." is optional; without alpha the scale is 1, with it alpha / rank
    assert ref["conv_in"][0].shape == (3, 4, 3, 3) and ref["conv_in"][1].shape == (64, 3, 1, 1)
    sd = {k[5:]: v for k, v in lora.synthetic_adapter(cfg, rank=3, seed=11).items()}
    canon, _ = lora.parse_state_dict(sd, cfg)
    assert all(v[2] is None for v in canon.values()) and torch.equal(canon["conv_out"][0], ref["conv_out"][0])
    st = _recorder(_tiny_unet())
    st.add("a", canon)
    assert {c[2] for _, cols in st.layout for c in cols} == {1.0} and set(st.calls[-1].tolist()) == {1.0}
    st.add("b", ref)
    assert {c[2] for _, cols in st.layout for c in cols if c[0] == "b"} == {0.5}


def test_name_tables_against_the_sdxl_manifest():
    from imagharmony_amd import lora
    from imagharmony_amd.unet import UNetConfig
    man = _manifest_weights()
    t_dif, t_sgm = lora.name_tables(UNetConfig())
    assert len(man) == 794
    for tab in (t_dif, t_sgm):
        assert set(tab.values()) <= set(man)                       # every module name the tables produce occurs in the manifest
        assert len(set(tab.values())) == len(tab)                   # no two entries map to one module
        assert set(tab.values()) == set(man)                        # every Linear / Conv weight of the manifest has an entry
    assert len(set(t_sgm) | set(t_dif)) == 2 * len(man)             # (the two key spaces do not collide)
    shapes = {n: tuple(m.weight.shape) for n, m in lora.adaptable_modules(lora._meta_unet(UNetConfig())).items()}
    assert shapes == man
    # the published SGM layout, by hand
    want = {"input_blocks_0_0": "conv_in", "input_blocks_1_0_in_layers_2": "down_blocks.0.resnets.0.conv1",
            "input_blocks_2_0_emb_layers_1": "down_blocks.0.resnets.1.time_emb_proj", "input_blocks_3_0_op": "down_blocks.0.downsamplers.0.conv",
            "input_blocks_6_0_op": "down_blocks.1.downsamplers.0.conv", "input_blocks_4_0_skip_connection": "down_blocks.1.resnets.0.conv_shortcut",
            "input_blocks_4_1_transformer_blocks_0_attn1_to_q": "down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_q",
            "input_blocks_5_1_proj_in": "down_blocks.1.attentions.1.proj_in", "input_blocks_7_0_out_layers_3": "down_blocks.2.resnets.0.conv2",
            "input_blocks_8_1_transformer_blocks_9_ff_net_0_proj": "down_blocks.2.attentions.1.transformer_blocks.9.ff.net.0.proj",
            "middle_block_0_in_layers_2": "mid_block.resnets.0.conv1", "middle_block_1_proj_out": "mid_block.attentions.0.proj_out",
            "middle_block_2_out_layers_3": "mid_block.resnets.1.conv2", "output_blocks_0_0_skip_connection": "up_blocks.0.resnets.0.conv_shortcut",
            "output_blocks_2_1_transformer_blocks_3_attn2_to_out_0": "up_blocks.0.attentions.2.transformer_blocks.3.attn2.to_out.0",
            "output_blocks_2_2_conv": "up_blocks.0.upsamplers.0.conv", "output_blocks_5_2_conv": "up_blocks.1.upsamplers.0.conv",
            "output_blocks_3_1_transformer_blocks_1_ff_net_2": "up_blocks.1.attentions.0.transformer_blocks.1.ff.net.2",
            "output_blocks_8_0_in_layers_2": "up_blocks.2.resnets.2.conv1", "time_embed_0": "time_embedding.linear_1",
            "time_embed_2": "time_embedding.linear_2", "label_emb_0_0": "add_embedding.linear_1", "label_emb_0_2": "add_embedding.linear_2",
            "out_2": "conv_out"}
    for k, v in want.items():
        assert t_sgm["lora_unet_" + k] == v, k
    assert t_dif["lora_unet_down_blocks_1_attentions_0_transformer_blocks_0_attn1_to_q"] == "down_blocks.1.attentions.0.transformer_blocks.0.attn1.to_q"


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_name_the_key_and_change_nothing():
    from imagharmony_amd import lora
    cfg = _tiny_cfg()
    u = _tiny_unet()
    base = lora.synthetic_adapter(cfg, rank=2, seed=1, select=lambda n: n.endswith("attn1.to_q"), naming="kohya")
    stem = next(iter(base)).split(".")[0]
    w = torch.zeros(2, 2)
    before = {k: v.clone() for k, v in u.state_dict().items()}
    for key in (stem + ".dora_scale", stem + ".hada_w1_a", stem + ".lokr_w1", stem + ".lora_mid.weight", stem + ".bias",
                "lora_te1_text_model_encoder_layers_0_mlp_fc1.lora_down.weight", "text_encoder.text_model.encoder.layers.0.mlp.fc1.lora_A.weight"):
        with pytest.raises(NotImplementedError) as e:
            u.load_lora_weights(dict(base, **{key: w}))
        assert key in str(e.value)
    for bad in ("lora_unet_input_blocks_99_0.lora_down.weight", "unet.nowhere.to_q.lora_A.weight", "some.other.key"):
        with pytest.raises(KeyError) as e:
            u.load_lora_weights(dict(base, **{bad: w}))
        assert bad in str(e.value)
    half = {k: v for k, v in base.items() if not k.endswith("lora_up.weight")}
    with pytest.raises(KeyError, match="one factor"):
        u.load_lora_weights(half)
    # factor shapes that do not fit the module (KeyError naming it), through a state whose device side is a recorder
    st = _recorder(u)
    canon, _ = lora.parse_state_dict(base, cfg)
    mod = next(iter(canon))
    wrong = dict(canon)
    wrong[mod] = (canon[mod][0][:, :-1], canon[mod][1], None)
    with pytest.raises(KeyError) as e:
        st.add("x", wrong)
    assert mod in str(e.value) and st.adapters == {} and st.snap == {} and st.calls == []
    # per-block adapter-weight dicts
    st.add("x", canon)
    with pytest.raises(NotImplementedError, match="per-block"):
        st.set_adapters(["x"], [{"down": 1.0}])
    assert len(st.calls) == 1
    # text-encoder keys under "skip": left out, listed
    te = "lora_te2_text_model_encoder_layers_3_self_attn_q_proj.lora_up.weight"
    canon2, skipped = lora.parse_state_dict(dict(base, **{te: w}), cfg, text_encoder="skip")
    assert skipped == [te] and list(canon2) == list(canon)
    # a UNet whose weights are not on the GPU in bf16 / fp16: ValueError before anything changes
    with pytest.raises(ValueError, match="bf16 / fp16"):
        u.load_lora_weights(base)
    with pytest.raises(ValueError, match="no LoRA is loaded"):
        u.set_adapters(["x"])
    with pytest.raises(NotImplementedError):
        u.unfuse_lora()
    assert u._lora is None and u.lora_epoch == 0 and u.get_list_adapters() == [] and u.get_active_adapters() == []
    after = u.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
    assert all(p._version == 1 for p in u.parameters())             # (the zero fill of _tiny_unet, nothing since)


def test_pipeline_methods_delegate_and_engine_guard_is_host_logic():
    """the pipeline classes inherit the LoRA methods and hand them to the UNet; the engine compares unet.lora_epoch with what
    set_conditioning saw"""
    import imagharmony_amd as ia
    from imagharmony_amd.denoise import DenoiseEngine
    from imagharmony_amd.lora import LoRAMixin, LoRAPipelineMixin
    from imagharmony_amd.unet import UNet2DConditionModel
    names = ("load_lora_weights", "set_adapters", "get_active_adapters", "get_list_adapters", "delete_adapters", "disable_lora", "enable_lora",
             "unload_lora_weights", "fuse_lora", "unfuse_lora")
    assert issubclass(UNet2DConditionModel, LoRAMixin) and all(hasattr(UNet2DConditionModel, n) for n in names)
    for cls in ia._PIPELINES:
        assert issubclass(getattr(ia, cls), LoRAPipelineMixin) and all(hasattr(getattr(ia, cls), n) for n in names)
    from imagharmony_amd.controlnet import ControlNetModel
    assert not hasattr(ControlNetModel, "load_lora_weights")

    class U:
        lora_epoch = 0
    class Cond:                 # the context that owns the conditioning's caches carries the epoch they were computed at
        weights_epoch = 0
    eng = DenoiseEngine(U(), "cpu")
    eng._check_weights_epoch()  # no conditioning yet: nothing to be stale
    eng._cond_ctx = Cond()
    eng._check_weights_epoch()
    eng.unet.lora_epoch = 1
    with pytest.raises(RuntimeError, match="weights changed since set_conditioning"):
        eng._check_weights_epoch()
    with pytest.raises(RuntimeError, match="weights changed since set_conditioning"):
        eng.set_schedule(None, 4)
    with pytest.raises(RuntimeError, match="weights changed since set_conditioning"):
        eng.denoise(None)


# ---------------------------------------------------------------------------------------------------- bookkeeping
def test_bookkeeping_factor_order_and_strengths():
    from imagharmony_amd import lora
    cfg = _tiny_cfg()
    u = _tiny_unet()
    st = _recorder(u)
    q = lambda n: n.endswith("attn1.to_q")
    qk = lambda n: n.endswith(("attn1.to_q", "attn1.to_k")) or n == "conv_in"
    a, _ = lora.parse_state_dict(lora.synthetic_adapter(cfg, rank=2, seed=1, select=qk, alpha=4.0), cfg)      # alpha / rank = 2
    b, _ = lora.parse_state_dict(lora.synthetic_adapter(cfg, rank=3, seed=2, select=q), cfg)                  # no alpha: 1
    st.add("A", a)
    st.add("B", b)
    order = [n for n in lora.adaptable_modules(u) if qk(n)]
    assert [m for m, _ in st.layout] == order and order[0] == "conv_in"
    off = 0
    for mod, cols in st.layout:                                      # offsets run through the layout; A's columns come before B's
        want = [("A", 2, 2.0)] + ([("B", 3, 1.0)] if q(mod) else [])
        assert [c[:3] for c in cols] == want
        for c in cols:
            assert c[3] == off
            off += c[1]
        U, D = st.factors(mod)
        assert U.shape == (a[mod][1].shape[0], sum(c[1] for c in cols)) and D.shape[0] == U.shape[1]
        assert torch.equal(D[:2], a[mod][0].reshape(2, -1)) and torch.equal(U[:, :2], a[mod][1].reshape(-1, 2))
        if q(mod):
            assert torch.equal(D[2:], b[mod][0]) and torch.equal(U[:, 2:], b[mod][1])
    assert off == len(st.g_host)

    def g_of(wa, wb):
        out = []
        for mod, cols in st.layout:
            out += [wa * 2.0] * 2 + ([wb * 1.0] * 3 if q(mod) else [])
        return np.array(out, dtype=np.float32)
    assert len(st.calls) == 2 and np.array_equal(st.calls[-1], g_of(1.0, 1.0))
    st.set_adapters(["A", "B"], [0.7, -0.3])
    assert np.array_equal(st.calls[-1], g_of(0.7, -0.3)) and st.active() == ["A", "B"]
    st.set_adapters("B")                                             # A becomes inactive: 0, B back at weight 1
    assert np.array_equal(st.calls[-1], g_of(0.0, 1.0)) and st.active() == ["B"]
    st.set_enabled(False)
    assert not st.calls[-1].any() and st.active() == []
    st.set_enabled(True)
    assert np.array_equal(st.calls[-1], g_of(0.0, 1.0))
    st.set_adapters(["A", "B"], [0.5, 2.0])
    n = len(st.calls)
    st.delete("B")                                                   # the layout shrinks; every snapshotted module keeps its item
    assert len(st.calls) == n + 1 and [m for m, _ in st.layout] == order and all([c[0] for c in cols] == ["A"] for _, cols in st.layout)
    assert np.array_equal(st.calls[-1], np.full(2 * len(order), 1.0, np.float32))
    st.delete(["A"])
    assert [cols for _, cols in st.layout] == [[]] * len(order) and len(st.calls[-1]) == 0 and set(st.snap) == set(order)
    with pytest.raises(ValueError, match="no adapter"):
        st.delete("A")
    with pytest.raises(ValueError, match="adapter_weights"):
        st.set_adapters([], [1.0])


# ---------------------------------------------------------------------------------------------------- header, binding, argument refusals
def test_header_declares_and_binds_the_two_entries():
    from imagharmony_amd import lib as L
    l = L.load()
    hdr = open(os.path.join(ROOT, "include", "imh_lora.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert "IMH_ABI_VERSION" not in code and '#include "imh.h"' in hdr and "enum" not in code and "Memory:" in hdr
    assert set(re.findall(r"\b(imh_[a-z0-9_]+)\s*\(", code)) == {"imh_lora_merge", "imh_lora_merge_tiles"} == {n for n, _, _ in L.LORA_SYMBOLS}
    assert all(hasattr(l, n) for n, _, _ in L.LORA_SYMBOLS)
    for cname, struct in (("imh_lora_item", L.LoraItem), ("imh_lora_merge_args", L.LoraMergeArgs)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), code, re.S).group(1)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                parts = decl.replace("*", " ").split(",")
                names.append(parts[0].split()[-1])
                names.extend(p.strip() for p in parts[1:])
        assert names == [f[0] for f in struct._fields_], cname
    assert C.sizeof(L.LoraItem) == 72
    assert l.imh_lora_merge_tiles(1, 1) == 1 and l.imh_lora_merge_tiles(128, 128) == 1 and l.imh_lora_merge_tiles(129, 257) == 6
    assert l.imh_lora_merge_tiles(0, 5) == 0 and l.imh_lora_merge_tiles(5, -1) == 0
    # not a plan kind
    p = l.imh_plan_create()
    a = L.LoraMergeArgs()
    for kind in (12, 14, 16, 18):
        assert l.imh_plan_add(p, kind, C.byref(a), 0, 0) < 0
    l.imh_plan_destroy(p)


def lora_refusals(base):
    """every argument refusal of include/imh_lora.h as (status, overrides of the item, overrides of the args); shared with the GPU test"""
    return [(-1, dict(base=None), {}), (-1, dict(dst=None), {}), (-1, dict(U=None), {}), (-1, dict(D=None), {}), (-1, dict(g=None), {}),
            (-1, {}, dict(items_host=None)), (-1, {}, dict(items_dev=None)), (-1, {}, dict(tile_start_dev=None)),
            (-1, dict(base=base + 1), {}), (-1, dict(dst=base + 8192 + 1), {}), (-1, dict(U=base + 16384 + 2), {}),
            (-1, dict(D=base + 24576 + 1), {}), (-1, dict(g=base + 28672 + 2), {}),
            (-1, dict(dst=base + 2), {}), (-1, dict(dst=base + 16384 + 4), {}), (-1, dict(dst=base + 24576 + 4), {}), (-1, dict(dst=base + 28672), {}),
            (-2, dict(N=0), {}), (-2, dict(K=0), {}), (-2, dict(N=-3), {}), (-2, dict(R=-1), {}),
            (-2, dict(ld_base=7), {}), (-2, dict(ld_dst=7), {}), (-2, dict(ldu=1), {}), (-2, dict(ldd=7), {}),
            (-2, dict(N=1 << 20, ld_dst=1 << 11, ld_base=1 << 11), {}), (-2, {}, dict(total_tiles=2)), (-2, {}, dict(n_items=0)),
            (-3, {}, dict(dtype=2)), (-3, {}, dict(dtype=-1))]


def test_merge_argument_errors_are_status_codes():
    from imagharmony_amd import lib as L
    l = L.load()
    buf = (C.c_char * 40960)()
    base = (C.addressof(buf) + 15) & ~15

    def call(item, args):
        it = (L.LoraItem * 1)()
        it[0].base, it[0].dst, it[0].U, it[0].D, it[0].g = base, base + 8192, base + 16384, base + 24576, base + 28672
        it[0].N, it[0].K, it[0].R, it[0].ld_base, it[0].ld_dst, it[0].ldu, it[0].ldd = 4, 8, 2, 8, 8, 2, 8
        for k, v in item.items():
            setattr(it[0], k, v)
        a = L.LoraMergeArgs()
        a.items_host, a.items_dev, a.tile_start_dev, a.n_items, a.total_tiles, a.dtype = C.addressof(it), base + 32768, base + 36864, 1, 1, 0
        for k, v in args.items():
            setattr(a, k, v)
        return l.imh_lora_merge(C.byref(a), None)
    assert l.imh_lora_merge(None, None) == -1
    for rc, item, args in lora_refusals(base):
        assert call(item, args) == rc, (item, args, l.imh_last_error())
    assert call(dict(dst=base + 2), {}) == -1 and b"overlap" in l.imh_last_error()
