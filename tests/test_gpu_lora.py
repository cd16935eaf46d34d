"""GPU: LoRA merged into the SDXL UNet's weights (imagharmony_amd.lora, include/imh_lora.h, csrc/lora.hip) -- the grouped merge kernel
against the float64 formula under guarded placement, the derived weight copies after a merge (no stale copy), several adapters, and the
pipeline / engine / PNS surface on the tiny stack.

The bound of every element, derived and not measured: with x the float64 value of W0 + sum_j U g D,
    |out - x| <= 0.5 ulp_T(max(|x|, |out|)) + (R + 3) 2^-24 (|W0| + sum_j |U g D|)
-- one fp32 rounding of g * D, R fp32 accumulations, the add of the base and the rounding to T."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle.detfill import det_fill, det_randn

from test_gpu_unet import build_pair, inputs
from test_lora_host import lora_refusals

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
# (N, K, R, ld_base, ld_dst, ldu, ldd): ld_dst > K everywhere; even / odd leading dimensions take the paired / the element-wise accesses
ITEMS = [(1, 1, 1, 1, 4, 1, 1), (65, 72, 3, 72, 76, 4, 72), (128, 64, 0, 64, 67, 0, 64), (64, 320, 130, 321, 328, 130, 320), (257, 129, 16, 130, 133, 16, 132)]


def _bits(t):
    return t.contiguous().view(torch.int16)


def _ulp(v, dtype):
    """the spacing of T at |v| (float64 tensor), subnormals included"""
    p, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    _, e = torch.frexp(v.abs())
    e = torch.where(v == 0, torch.full_like(e, emin + 1), e)
    return torch.ldexp(torch.ones_like(v), torch.clamp(e - 1, min=emin) - p)


def _check_bound(out, w0, U, D, g, dtype, what=""):
    """out, w0: T; U [N, R], D [R, K], g [R]: fp32 (or None at rank 0) -- every element within the derived bound of the float64 formula"""
    o, b = out.double().cpu(), w0.double().cpu()
    if U is None or U.shape[1] == 0:
        x, ab, R = b, b.abs(), 0
    else:
        gd = g.double().cpu()[:, None] * D.double().cpu()
        x, ab, R = b + U.double().cpu() @ gd, b.abs() + U.double().cpu().abs() @ gd.abs(), U.shape[1]
    bound = 0.5 * _ulp(torch.maximum(x.abs(), o.abs()), dtype) + (R + 3) * 2.0 ** -24 * ab
    err = (o - x).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: max |out - x| / bound = {worst:.3f} (R = {R})")
    assert bool((err <= bound).all()), (what, worst)


@functools.lru_cache(maxsize=None)
def _item_data(dtype):
    """per item (base T [N, K], U fp32 [N, R], D fp32 [R, K], g fp32 [R]) on the CPU, computed once"""
    out = []
    for i, (N, K, R, *_rest) in enumerate(ITEMS):
        base = det_randn((N, K), 40 + i).mul(0.05).to(dtype)
        base.view(-1)[::7] = -0.0                                      # a zero sum must leave these bits alone
        rnd = lambda shape, seed: det_randn(shape, seed) if R else torch.zeros(shape)      # noqa: E731
        out.append((base, rnd((N, R), 50 + i), rnd((R, K), 60 + i).mul(0.1), rnd((R,), 70 + i).mul(0.5)))
    return out


def _launch(dtype, which, g_zero=False):
    """one grouped launch over the items `which` inside a guarded arena -> ([dst views], arena)"""
    from guarded import Arena
    from imagharmony_amd import lib as L
    lib = L.load()
    data = _item_data(dtype)
    specs = []
    for i in which:
        N, K, R, ldb, ldd_, ldu, ldD = ITEMS[i]
        specs += [((N, K), dtype, ldb), ((N, K), dtype, ldd_), ((N, max(R, 1)), torch.float32, max(ldu, 1)), ((max(R, 1), K), torch.float32, ldD),
                  ((max(R, 1),), torch.float32, None)]
    specs += [((72 * len(which),), torch.uint8, None), ((len(which) + 1,), torch.int32, None)]
    arena = Arena(DEV, Arena.size_for(specs))
    items = (L.LoraItem * len(which))()
    dsts, prefix = [], [0]
    for n, i in enumerate(which):
        N, K, R, ldb, ldd_, ldu, ldD = ITEMS[i]
        base, U, D, g = data[i]
        vb = arena.place(base, ld=ldb, name=f"base{i}")
        vd = arena.carve((N, K), dtype, ld=ldd_, role="out", name=f"dst{i}")
        it = items[n]
        it.base, it.dst, it.N, it.K, it.R, it.ld_base, it.ld_dst, it.ldu, it.ldd = vb.data_ptr(), vd.data_ptr(), N, K, R, ldb, ldd_, ldu, ldD
        if R:
            vu, vD = arena.place(U, ld=ldu, name=f"U{i}"), arena.place(D, ld=ldD, name=f"D{i}")
            vg = arena.place(torch.zeros_like(g) if g_zero else g, name=f"g{i}")
            it.U, it.D, it.g = vu.data_ptr(), vD.data_ptr(), vg.data_ptr()
        dsts.append(vd)
        prefix.append(prefix[-1] + lib.imh_lora_merge_tiles(N, K))
    tab = arena.place(torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8), name="items")
    pre = arena.place(torch.tensor(prefix, dtype=torch.int32), name="prefix")
    a = L.LoraMergeArgs()
    a.items_host, a.items_dev, a.tile_start_dev, a.n_items, a.total_tiles = C.addressof(items), tab.data_ptr(), pre.data_ptr(), len(which), prefix[-1]
    a.dtype = L.IMH_DT_BF16 if dtype == torch.bfloat16 else L.IMH_DT_F16
    L.check(lib.imh_lora_merge(C.byref(a), torch.cuda.current_stream().cuda_stream), "imh_lora_merge")
    torch.cuda.synchronize()
    arena.check()                                                     # no byte outside the dst rows changed (the gaps [K, ld_dst) included); dst is finite
    return dsts, arena


@pytest.mark.parametrize("dtype", DTYPES)
def test_grouped_merge_matches_the_formula_under_guards(dtype):
    data = _item_data(dtype)
    every = list(range(len(ITEMS)))
    dsts, _ = _launch(dtype, every)
    outs = [d.clone() for d in dsts]
    for i, out in enumerate(outs):
        base, U, D, g = data[i]
        _check_bound(out, base, U, D, g, dtype, f"item {ITEMS[i][:3]} {dtype}")
        if ITEMS[i][2] == 0:
            assert torch.equal(_bits(out.cpu()), _bits(base))          # rank 0: a copy
        else:
            assert not torch.equal(_bits(out.cpu()), _bits(base))
    again, _ = _launch(dtype, every)                                    # the same bits on every call
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(again, outs))
    for i in every:                                                     # each item alone: the bits of the grouped launch
        alone, _ = _launch(dtype, [i])
        assert torch.equal(_bits(alone[0]), _bits(outs[i])), ITEMS[i]
    zero, _ = _launch(dtype, every, g_zero=True)                        # g == 0: the base's bits, -0 included
    assert all(torch.equal(_bits(z.cpu()), _bits(data[i][0])) for i, z in enumerate(zero))


def test_many_items_find_their_tiles():
    """600 items, one or two tiles each: a workgroup's 256-way search for its item takes a second round beyond 256 items; every item
    gets the bits it gets in a launch of its own group of 100 (one round), and the formula holds"""
    from imagharmony_amd import lib as L
    lib = L.load()
    dtype, M, NM, K, R = torch.bfloat16, 600, 130, 5, 2
    rows = [NM if i % 7 == 3 else 1 + i % 3 for i in range(M)]
    base = det_randn((M, NM, K), 80).mul(0.05).to(dtype).to(DEV)
    U, D, g = det_randn((M, NM, R), 81).to(DEV), det_randn((M, R, K), 82).mul(0.1).to(DEV), det_randn((M, R), 83).to(DEV)

    def launch(which):
        dst = torch.zeros_like(base)
        items = (L.LoraItem * len(which))()
        prefix = [0]
        for n, i in enumerate(which):
            it = items[n]
            it.base, it.dst, it.U, it.D, it.g = base[i].data_ptr(), dst[i].data_ptr(), U[i].data_ptr(), D[i].data_ptr(), g[i].data_ptr()
            it.N, it.K, it.R, it.ld_base, it.ld_dst, it.ldu, it.ldd = rows[i], K, R, K, K, R, K
            prefix.append(prefix[-1] + lib.imh_lora_merge_tiles(rows[i], K))
        tab = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(DEV)
        pre = torch.tensor(prefix, dtype=torch.int32, device=DEV)
        a = L.LoraMergeArgs()
        a.items_host, a.items_dev, a.tile_start_dev, a.n_items, a.total_tiles = C.addressof(items), tab.data_ptr(), pre.data_ptr(), len(which), prefix[-1]
        a.dtype = L.IMH_DT_BF16
        L.check(lib.imh_lora_merge(C.byref(a), torch.cuda.current_stream().cuda_stream), "imh_lora_merge")
        torch.cuda.synchronize()
        return dst
    whole = launch(list(range(M)))
    parts = sum(launch(list(range(s, s + 100))).float() for s in range(0, M, 100))      # (rows no item covers stay zero)
    assert torch.equal(whole.float(), parts)
    for i in (0, 3, 255, 256, 257, 599):
        _check_bound(whole[i, :rows[i]], base[i, :rows[i]], U[i, :rows[i]], D[i], g[i], dtype, f"item {i} of {M}")
        assert not whole[i, rows[i]:].any() and whole[i, :rows[i]].float().abs().sum() > 0


def test_merge_refusals_launch_nothing():
    from imagharmony_amd import lib as L
    lib = L.load()
    buf = torch.full((40960 + 16,), 0x5A, dtype=torch.uint8, device=DEV)
    base = (buf.data_ptr() + 15) & ~15
    keep = buf.clone()

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
        return lib.imh_lora_merge(C.byref(a), torch.cuda.current_stream().cuda_stream)
    assert lib.imh_lora_merge(None, None) == -1
    for rc, item, args in lora_refusals(base):
        assert call(item, args) == rc, (item, args)
    torch.cuda.synchronize()
    assert torch.equal(buf, keep)


# ---------------------------------------------------------------------------------------------------- the UNet
def _call_unet(hu, ocfg, dtype):
    x, ehs, te, ids = inputs(ocfg)
    return hu(x.to(DEV), torch.tensor(500.0), ehs.to(DEV, dtype), added_cond_kwargs={"text_embeds": te.to(DEV, dtype), "time_ids": ids.to(DEV)})[0].clone()


def _weights(hu):
    from imagharmony_amd.lora import adaptable_modules
    return {n: m.weight.detach().clone() for n, m in adaptable_modules(hu).items()}


def test_no_stale_copy_after_load_and_unload():
    """a forward builds every derived copy (packed convs, the phase form, the GEGLU interleave, folded LayerNorms, [Q|K|V], the stacked
    time_emb_proj); after a load the next forward must be the one of a fresh UNet that got the merged master weights"""
    from imagharmony_amd import lora
    dtype = torch.bfloat16
    _, hu, ocfg = build_pair(dtype)
    w0 = _weights(hu)
    y0 = _call_unet(hu, ocfg, dtype)
    rep = hu.load_lora_weights(lora.synthetic_adapter(hu, rank=4, seed=3, std=0.05, alpha=8.0), adapter_name="style")
    assert rep["adapter_name"] == "style" and rep["rank"] == 4 and rep["skipped"] == [] and rep["modules"] == list(w0)
    for must in ("conv_in", "conv_out", "time_embedding.linear_1", "add_embedding.linear_2", "down_blocks.1.resnets.0.conv_shortcut",
                 "up_blocks.0.upsamplers.0.conv", "down_blocks.0.downsamplers.0.conv", "mid_block.attentions.0.transformer_blocks.0.ff.net.0.proj",
                 "down_blocks.0.resnets.0.time_emb_proj"):
        assert must in rep["modules"]
    assert hu.lora_epoch == 1 and hu.get_active_adapters() == ["style"] and hu.get_list_adapters() == ["style"]
    w1 = _weights(hu)
    assert all(not torch.equal(w1[n], w0[n]) for n in w0)
    y1 = _call_unet(hu, ocfg, dtype)
    _, fresh, _ = build_pair(dtype)
    fresh.load_state_dict(hu.state_dict())
    assert torch.equal(y1, _call_unet(fresh, ocfg, dtype)) and not torch.equal(y1, y0) and torch.isfinite(y1).all()
    hu.unload_lora_weights()
    assert hu._lora is None and hu.lora_epoch == 2 and hu.get_list_adapters() == []
    w2 = _weights(hu)
    assert all(torch.equal(_bits(w2[n]), _bits(w0[n])) for n in w0)
    assert torch.equal(_call_unet(hu, ocfg, dtype), y0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_adapters_weights_and_switches(dtype):
    from imagharmony_amd import lora
    _, hu, ocfg = build_pair(dtype)
    w0 = _weights(hu)
    sel = lambda n: n.endswith(("to_q", "to_out.0", "ff.net.2", "conv1", "proj_in")) or n in ("conv_in", "conv_out")
    sd_a = lora.synthetic_adapter(hu, rank=4, seed=5, std=0.05, alpha=2.0, select=sel, naming="sgm")
    sd_b = lora.synthetic_adapter(hu, rank=6, seed=6, std=0.05, select=lambda n: sel(n) and "attn2" not in n, naming="kohya")
    hu.load_lora_weights(sd_a, adapter_name="a")
    only_a = _weights(hu)
    hu.load_lora_weights(sd_b, adapter_name="b")
    hu.set_adapters(["a", "b"], [0.7, -0.3])
    st = hu._lora
    got = _weights(hu)
    touched = [m for m, _ in st.layout]
    assert touched == [n for n in w0 if sel(n)]
    for mod, cols in st.layout:
        U, D = st.factors(mod)
        g = torch.from_numpy(st.g_host[cols[0][3]:cols[0][3] + U.shape[1]].copy())
        want_g = [np.float32(0.7 * 0.5)] * 4 + ([np.float32(-0.3)] * 6 if len(cols) == 2 else [])
        assert g.tolist() == [float(v) for v in want_g]
        _check_bound(got[mod].reshape(U.shape[0], -1), w0[mod].reshape(U.shape[0], -1), U, D, g, dtype, mod)
    assert all(torch.equal(_bits(got[n]), _bits(w0[n])) for n in w0 if n not in touched)
    hu.set_adapters(["a", "b"], [1.0, 0.0])                            # equals loading the first alone, bit for bit
    assert all(torch.equal(_bits(v), _bits(only_a[n])) for n, v in _weights(hu).items())
    hu.set_adapters("a")
    assert hu.get_active_adapters() == ["a"] and all(torch.equal(_bits(v), _bits(only_a[n])) for n, v in _weights(hu).items())
    hu.disable_lora()
    assert hu.get_active_adapters() == [] and all(torch.equal(_bits(v), _bits(w0[n])) for n, v in _weights(hu).items())
    hu.enable_lora()
    hu.delete_adapters("b")
    assert hu.get_list_adapters() == ["a"] and all(torch.equal(_bits(v), _bits(only_a[n])) for n, v in _weights(hu).items())
    hu.delete_adapters("a")                                             # the last adapter: rank-0 items copy the snapshots back
    assert hu.get_list_adapters() == [] and all(torch.equal(_bits(v), _bits(w0[n])) for n, v in _weights(hu).items())
    hu.load_lora_weights(sd_a, adapter_name="a")
    hu.fuse_lora()                                                      # the merged weights stay, the state goes
    assert hu._lora is None and all(torch.equal(_bits(v), _bits(only_a[n])) for n, v in _weights(hu).items())
    with pytest.raises(NotImplementedError):
        hu.unfuse_lora()
    with pytest.raises(ValueError, match="bf16 / fp16"):               # fp32 weights on the GPU: refused before anything changes
        hu.float().load_lora_weights(sd_a)


# ---------------------------------------------------------------------------------------------------- pipeline, engine, PNS
T_TOKENS = 4
SEEDS = [3, 9]


def _loop_inputs(ocfg, S=1):
    cd = ocfg.cross_attention_dim
    return (det_randn((S, 4, 32, 32), 3), det_randn((S, 77 + T_TOKENS, cd), 4), det_randn((S, 77 + T_TOKENS, cd), 5),
            det_randn((S, ocfg.pooled_dim), 6), det_randn((S, ocfg.pooled_dim), 7))


def _kinds(plan):
    return [plan.lib.imh_plan_get_kind(plan.plan, i) for i in range(plan.lib.imh_plan_size(plan.plan))]


def _scorer(lat):
    from imagharmony_amd import pns
    return torch.cat([pns.default_scorer(lat[k:k + 1].float().cpu()) for k in range(lat.shape[0])])


def test_pipeline_engine_guard_and_pns():
    from imagharmony_amd import StableDiffusionXLCustomPipeline, lora
    from imagharmony_amd import schedulers as hs
    from imagharmony_amd.denoise import DenoiseEngine
    from imagharmony_amd.ip_adapter import IPAdapterXL
    from imagharmony_amd.modules import HarmonyAttention
    dtype = torch.bfloat16
    _, hu, ocfg = build_pair(dtype, num_tokens=T_TOKENS)
    lat, pe, ne, po, no = _loop_inputs(ocfg)
    pipe = StableDiffusionXLCustomPipeline(hu, scheduler=hs.DDIMScheduler(), device=DEV, dtype=dtype)
    call = dict(prompt_embeds=pe, negative_prompt_embeds=ne, pooled_prompt_embeds=po, negative_pooled_prompt_embeds=no, latents=lat,
                num_inference_steps=4, guidance_scale=5.0, output_type="latent")
    before = pipe(**call).images.clone()
    kinds0, tags0 = _kinds(pipe.engine.plan), [(t[1], t[2]) for t in pipe.engine.plan.tags]
    sd = lora.synthetic_adapter(hu, rank=4, seed=8, std=0.05, select=lambda n: lora.ATTN_FF_PROJ.search(n) is not None)
    rep = pipe.load_lora_weights(sd, adapter_name="style")
    assert rep["modules"] and pipe.get_active_adapters() == ["style"] and pipe.get_list_adapters() == {"unet": ["style"]}
    mid = pipe(**call).images.clone()
    # the recorded step: the same launches, op for op, with and without the adapter
    assert _kinds(pipe.engine.plan) == kinds0 and [(t[1], t[2]) for t in pipe.engine.plan.tags] == tags0
    _, hu2, _ = build_pair(dtype, num_tokens=T_TOKENS)
    hu2.load_state_dict(hu.state_dict())
    fresh = StableDiffusionXLCustomPipeline(hu2, scheduler=hs.DDIMScheduler(), device=DEV, dtype=dtype)
    assert torch.equal(mid, fresh(**call).images) and not torch.equal(mid, before) and torch.isfinite(mid).all()
    # an engine conditioned before a merge refuses to go on from its stale caches
    eng = DenoiseEngine(hu, DEV, dtype)
    eng.set_conditioning(pe, ne, po, no, 256, 256, guidance_scale=5.0)
    eng.set_schedule(hs.DDIMScheduler(), 4)
    pipe.set_adapters(["style"], [0.5])
    with pytest.raises(RuntimeError, match="weights changed since set_conditioning"):
        eng.set_schedule(hs.DDIMScheduler(), 4)
    with pytest.raises(RuntimeError, match="weights changed since set_conditioning"):
        eng.denoise(lat)
    eng.set_conditioning(pe, ne, po, no, 256, 256, guidance_scale=5.0)
    eng.set_schedule(hs.DDIMScheduler(), 4)
    half = eng.denoise(lat).clone()
    assert torch.equal(half, pipe(**call).images) and not torch.equal(half, mid)
    with pytest.raises(NotImplementedError, match="cross_attention_kwargs"):
        pipe(cross_attention_kwargs={"scale": 0.5}, **call)
    # PNS with the adapter loaded: the winner is the pipe's own call with that seed
    pipe.set_adapters(["style"], [1.0])
    cd = ocfg.cross_attention_dim
    ha = det_fill(HarmonyAttention(image_hidden_size=128, text_context_dim=cd, inter_dim=512, cross_heads=8, reshape_blocks=8, cross_value_dim=64), 3)
    ip = IPAdapterXL(pipe, None, None, DEV, num_tokens=T_TOKENS, inference=True, number_class_crossattention=ha, dtype=dtype, clip_embeddings_dim=128)
    det_fill(ip.image_proj_model, 5)
    for n, p in hu.attn_processors.items():
        det_fill(p, 9, prefix=n)
    embeds = (det_randn((1, 77, cd), 1), det_randn((1, 77, cd), 2), det_randn((1, ocfg.pooled_dim), 3), det_randn((1, ocfg.pooled_dim), 4))
    kw = dict(clip_image_embeds=det_randn((1, 128), 5), extra_prompt_embeds=det_randn((1, 77, cd), 6), guidance_scale=5.0)
    r = ip.generate_pns(SEEDS, preview_steps=2, num_inference_steps=4, batch=2, output_type="latent", scorer=_scorer, prompt_embeds=embeds, scale=0.8, **kw)
    win = r["latents"].to(DEV)
    assert r["best_seed"] in SEEDS and win.shape == (1, 4, 32, 32) and torch.isfinite(win).all()
    fused = ip.fused_clip_embeds(None, kw["clip_image_embeds"], kw["extra_prompt_embeds"])
    ipe, uipe = ip._g(ip.image_proj_model)(fused), ip._g(ip.image_proj_model)(torch.zeros_like(fused))
    direct = lambda: pipe(prompt_embeds=torch.cat([embeds[0].to(DEV, dtype), ipe], 1), negative_prompt_embeds=torch.cat([embeds[1].to(DEV, dtype), uipe], 1),      # noqa: E731
                          pooled_prompt_embeds=embeds[2], negative_pooled_prompt_embeds=embeds[3], num_inference_steps=4, guidance_scale=5.0,
                          output_type="latent", generator=[torch.Generator("cpu").manual_seed(int(r["best_seed"]))]).images
    with_lora = direct().float()
    assert torch.equal(with_lora, win)
    pipe.unload_lora_weights()
    assert not torch.equal(direct().float(), win)
    assert pipe.get_list_adapters() == {"unet": []}


def test_pipeline_unload_restores_the_first_latents():
    from imagharmony_amd import StableDiffusionXLCustomPipeline, lora
    from imagharmony_amd import schedulers as hs
    dtype = torch.float16
    _, hu, ocfg = build_pair(dtype, num_tokens=T_TOKENS)
    lat, pe, ne, po, no = _loop_inputs(ocfg)
    pipe = StableDiffusionXLCustomPipeline(hu, scheduler=hs.DDIMScheduler(), device=DEV, dtype=dtype)
    call = dict(prompt_embeds=pe, negative_prompt_embeds=ne, pooled_prompt_embeds=po, negative_pooled_prompt_embeds=no, latents=lat,
                num_inference_steps=4, guidance_scale=5.0, output_type="latent")
    first = pipe(**call).images.clone()
    pipe.load_lora_weights(lora.synthetic_adapter(hu, rank=2, seed=9, std=0.05, naming="sgm"))
    assert pipe.get_active_adapters() == ["default_0"]
    middle = pipe(**call).images.clone()
    pipe.unload_lora_weights()
    last = pipe(**call).images
    assert torch.equal(first, last) and not torch.equal(first, middle) and torch.isfinite(middle).all()
