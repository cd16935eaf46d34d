"""Preference-guided noise selection (PNS) sharded over the GPUs of one node.

The reference publishes the scheme only as a figure (README.md:27, assets/1.png): N candidate seeds ->
a short preview denoise each -> a judge scores the previews -> the best noise gets the full denoise.
The only code hook is the list-of-seeds generator (ip_adapter/utils.py:83-93).  Candidates are independent
trajectories (same weights, same conditioning, different initial noise), so the path shards with NO
per-step communication:

    rank r of W denoises seeds {i : i mod W == r};
    RCCL (torch.distributed backend "nccl") carries only: the one-time broadcast of the conditioning
    (and optionally of the weights, to guarantee identical replicas), the all_gather of N fp32 scores and
    the broadcast of the winning latent from its owner.

The judge is unpinned upstream (a VLM, no code); ``scorer`` is pluggable.  ``ClipPreferenceJudge`` is the
deterministic default of SURVEY.md 8f-2: decode the preview, embed it with the CLIP vision model the adapter
already holds, score = cosine similarity to the harmony-fused image embedding the denoise was conditioned on.
``default_scorer`` (a latent statistic) is the fallback when no VAE / CLIP model is attached.  Neither is a
quality claim; both are off the timed path of bench.py.
"""
from typing import Callable, List, Optional, Sequence

import torch
import torch.distributed as dist

from . import pipeline as _pipe


def default_scorer(latents: torch.Tensor) -> torch.Tensor:
    """[S, 4, h, w] -> [S] deterministic score (higher is better): negative deviation of the per-channel
    standard deviation from 1 -- a placeholder for the reference's VLM judge."""
    s = latents.float().flatten(2).std(dim=2)
    return -(s - 1.0).abs().mean(dim=1)


def shard(seeds: Sequence[int], rank: int, world: int) -> List[int]:
    return [s for i, s in enumerate(seeds) if i % world == rank]


def seed_latents(seed: int, shape) -> torch.Tensor:
    """backend-independent initial noise: drawn on a CPU generator (SURVEY.md 7 'RNG parity')"""
    return torch.randn(tuple(shape), generator=torch.Generator("cpu").manual_seed(int(seed)), dtype=torch.float32)


def broadcast_module_(module: torch.nn.Module, src: int = 0, bucket_bytes: int = 512 << 20):
    """one-time weight broadcast so every rank holds the same replica (RCCL over xGMI on GPUs).  The ~1700 parameter
    tensors of the UNet travel as a few flat buckets per dtype (xGMI is point-to-point: a handful of large ring
    broadcasts, not thousands of latency-bound small ones).  Returns the number of collectives issued."""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return 0
    rank = dist.get_rank()
    groups = {}
    for t in list(module.parameters()) + list(module.buffers()):
        if t.numel():
            groups.setdefault((t.dtype, t.device), []).append(t.data)
    n_coll = 0
    for (dtype, device), tensors in groups.items():
        bucket, size = [], 0
        esz = tensors[0].element_size()

        def flush():
            nonlocal bucket, size, n_coll
            if not bucket:
                return
            flat = torch.empty(size, dtype=dtype, device=device)
            off = 0
            if rank == src:
                for t in bucket:
                    flat[off:off + t.numel()].copy_(t.reshape(-1))
                    off += t.numel()
            dist.broadcast(flat, src=src)
            n_coll += 1
            if rank != src:
                off = 0
                for t in bucket:
                    t.copy_(flat[off:off + t.numel()].view_as(t))
                    off += t.numel()
            bucket, size = [], 0

        for t in tensors:
            if size and (size + t.numel()) * esz > bucket_bytes:
                flush()
            bucket.append(t)
            size += t.numel()
        flush()
    return n_coll


def broadcast_tensors_(tensors: Sequence[torch.Tensor], src: int = 0):
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        for t in tensors:
            dist.broadcast(t, src=src)


class ClipPreferenceJudge:
    """Default PNS judge (README.md:27 / assets/1.png name a VLM judge, no code): a candidate's
    preview latents are decoded (``decode_fn``: latents [S,4,h,w] -> images [S,3,H,W] in [-1,1], e.g.
    ``lambda z: decode_latents(vae, z)``), resized / normalised like CLIPImageProcessor does (bicubic to
    ``image_size``, centre crop, CLIP mean / std -- as tensor ops, so the score is reproducible bit for bit on one
    backend), embedded by the CLIP vision model (stock transformers module, the step before the path, 8f-4), and
    scored by cosine similarity with ``target_embeds`` -- the harmony-fused image embedding
    ``clip + HarmonyAttention(text, clip)`` (ip_adapter.py:170-173) the denoise was conditioned on."""

    from .imageops import CLIP_MEAN as MEAN, CLIP_STD as STD      # one set of constants for both preprocess backends

    def __init__(self, decode_fn, image_encoder, target_embeds, image_size=None, preprocess_backend="torch"):
        """preprocess_backend: "torch" (default) -- ``preprocess`` below, a chain of torch ops over the full-resolution images, then the
        encoder's ``forward``; "hip" -- ``CLIPVisionEncoder.embed_decoded``: one imh_clip_preprocess launch writes the encoder's patch rows
        from the decoded images (the same steps, specified in imagharmony_amd/imageops.py); needs a CLIPVisionEncoder (ValueError)."""
        if preprocess_backend not in ("torch", "hip"):
            raise ValueError(f"preprocess_backend={preprocess_backend!r}: 'torch' or 'hip'")
        if preprocess_backend == "hip" and not hasattr(image_encoder, "embed_decoded"):
            raise ValueError('preprocess_backend="hip" needs imagharmony_amd.clip_vision.CLIPVisionEncoder as the image encoder '
                             f"(got {type(image_encoder).__name__})")
        self.preprocess_backend = preprocess_backend
        self.decode_fn = decode_fn
        self.image_encoder = image_encoder
        cfg = getattr(image_encoder, "config", None)
        self.image_size = int(image_size or getattr(cfg, "image_size", 224))
        t = target_embeds.detach().float().reshape(-1, target_embeds.shape[-1])
        self.target = torch.nn.functional.normalize(t.mean(0, keepdim=True), dim=-1)

    @torch.no_grad()
    def preprocess(self, images):
        x = (images.float() / 2 + 0.5).clamp(0, 1)
        H, W = x.shape[-2:]
        sz = self.image_size
        sc = sz / min(H, W)                                   # shortest edge -> sz, then centre crop (CLIPImageProcessor)
        nh, nw = max(sz, round(H * sc)), max(sz, round(W * sc))
        x = torch.nn.functional.interpolate(x, size=(nh, nw), mode="bicubic", align_corners=False, antialias=True).clamp(0, 1)
        t, l = (nh - sz) // 2, (nw - sz) // 2
        x = x[..., t:t + sz, l:l + sz]
        mean = torch.tensor(self.MEAN, device=x.device).view(1, 3, 1, 1)
        std = torch.tensor(self.STD, device=x.device).view(1, 3, 1, 1)
        return (x - mean) / std

    @torch.no_grad()
    def __call__(self, latents):
        images = self.decode_fn(latents)
        if self.preprocess_backend == "hip":
            emb = self.image_encoder.embed_decoded(images.float().to(self.image_encoder.device)).image_embeds.float()
            emb = torch.nn.functional.normalize(emb, dim=-1)
            return (emb * self.target.to(emb.device)).sum(-1)
        p = next(self.image_encoder.parameters())
        px = self.preprocess(images).to(device=p.device, dtype=p.dtype)
        emb = self.image_encoder(px).image_embeds.float()
        emb = torch.nn.functional.normalize(emb, dim=-1)
        return (emb * self.target.to(emb.device)).sum(-1)


def _stage_fns(engine, scheduler, preview_steps, final_steps, step_noise, schedule_kw, strength=None, prepare=None, inpaint=False):
    """(preview_fn, final_fn) of two_stage_fns and -- ``prepare`` given -- edit_two_stage_fns: per stage set_schedule, for an edit truncated
    by ``strength`` and followed by ``prepare(seeds, t_start)``, then the denoise: of the noise handed in, or (an edit) of what prepare
    left in the engine"""
    from .schedulers import get_timesteps
    if step_noise not in ("global", "seed"):
        raise ValueError(f'step_noise must be "global" or "seed", not {step_noise!r}')
    seeded, edit = step_noise == "seed", prepare is not None

    def run(steps, noise, seeds):
        kw = {"seeded_noise": True} if seeded else {}    # (unseeded text-to-image: today's calls, keyword for keyword)
        if edit:
            if seeds is None:
                raise ValueError("an edit candidate is defined by its seed: run_pns(..., pass_seeds=True)")
            seeds, noise = [int(s) for s in seeds], None
            scheduler.set_timesteps(steps)
            _, t_start = get_timesteps(scheduler, steps, strength)
            kw.update(t_start=t_start, inpaint=inpaint)
        engine.set_schedule(scheduler, steps, **kw, **schedule_kw)
        if edit:
            prepare(seeds, t_start)
        if seeded and engine.seeded:                     # (a deterministic sampler ignores the flag: it draws no noise)
            if seeds is None:
                raise ValueError('step_noise="seed" needs the candidates\' seeds: run_pns(..., pass_seeds=True)')
            return engine.denoise(noise, step_seeds=list(seeds)).clone()
        return engine.denoise(noise).clone()

    def preview(noise=None, seeds=None):
        return run(preview_steps, noise, seeds)

    def final(noise=None, seeds=None):
        return run(final_steps, noise, seeds)

    return preview, final


def two_stage_fns(engine, scheduler, preview_steps=10, final_steps=30, step_noise="global", **schedule_kw):
    """The two-stage schedule of assets/1.png on a ``DenoiseEngine`` whose conditioning is set: every candidate seed
    gets a ``preview_steps`` denoise ("+10 steps"), the judged-best noise the full ``final_steps`` one ("+30 steps").
    Returns (preview_fn, final_fn) for ``run_pns``.
    Under a stochastic scheduler (SDE-DPM-Solver++, Euler ancestral) ``step_noise`` says where the per-step noise comes from:
    "global" (the default, today's behaviour): the engine is handed no generator, each denoise draws its noise bank from torch's global
    generator, so a candidate seed fixes the initial noise only -- the preview and the final run of the chosen seed use unrelated step
    noise, a seed does not reproduce its latent, and ranks differ;
    "seed": the schedules are seeded (DenoiseEngine.set_schedule(seeded_noise=True)) and every candidate's step noise is generated on
    the device from its own seed with lane 0 -- a seed then reproduces its latent alone or stacked, on any rank, and its preview and
    final run read the same noise rows 0 .. preview_steps - 1 (at different sigmas).  The functions then take ``seeds=`` (the
    candidates' seeds in stacking order): use ``run_pns(..., pass_seeds=True)``.
    The deterministic samplers (DDIM, Euler, DPM++ 2M with or without Karras sigmas) draw no noise and are unaffected either way.
    ``schedule_kw`` goes to set_schedule at both stages: the IP-scale window and, on an engine with a ControlNet and its control image
    set, ``controlnet_guidance_start / controlnet_guidance_end`` (counted per stage over the steps that run)."""
    return _stage_fns(engine, scheduler, preview_steps, final_steps, step_noise, schedule_kw)


def edit_draws(seeds, h, w, third=False):
    """what a candidate seed means in an edit: per seed the draws of the image-to-image / inpainting pipelines, in their order, from
    ``torch.Generator("cpu").manual_seed(seed)`` -- the posterior noise of the image, the add-noise noise and, ``third`` (9-channel
    inpainting UNet), the posterior noise of the masked image.  -> (n1, n2, n3 or None), each fp32 [len(seeds), 4, h, w] on the CPU: the
    tensors ``pipe(..., generator=[that generator])`` draws for a batch of one, stacked."""
    return _pipe.edit_draws([torch.Generator("cpu").manual_seed(int(s)) for s in seeds], len(seeds), 1, int(h), int(w), Bm=1 if third else None)


def edit_prepare_fn(engine, scheduler, scaling, moments, h, w, strength, mask=None, masked_moments=None, concat=False):
    """``prepare(seeds, t_start)`` for ``edit_two_stage_fns``: draws every candidate's noise (edit_draws) and writes the stacked initial
    latents -- and, inpainting, the blend / conv_in state -- into the engine under its current schedule.  moments: the image's encoder
    moments (one image, every candidate reads it; None where nothing reads them: a 9-channel UNet at strength 1.0); mask: the latent mask
    [1, 1, h, w] (inpainting, else None); concat: a 9-channel UNet, with masked_moments the masked image's encoder moments."""
    def prepare(seeds, t_start):
        return _pipe.edit_prepare(engine, scheduler, t_start, scaling, moments, edit_draws(seeds, h, w, third=concat), mask,
                                  float(strength) == 1.0, masked_moments)

    return prepare


def edit_two_stage_fns(engine, scheduler, prepare, strength, preview_steps=10, final_steps=30, step_noise="global", inpaint=False, **schedule_kw):
    """two_stage_fns for an edit (image-to-image, inpainting): every candidate seed gets a ``preview_steps`` schedule truncated by
    ``strength`` as the pipelines truncate theirs, the judged-best seed the ``final_steps`` one.  Returns (preview_fn, final_fn) for
    ``run_pns(..., pass_seeds=True)``: the functions ignore the noise run_pns hands them (an edit's initial latents are not plain noise)
    and take the candidates' ``seeds=``.  Per stage: scheduler.set_timesteps(steps); t_start from schedulers.get_timesteps (a schedule that
    truncates to no step raises its ValueError); engine.set_schedule(..., t_start=t_start, inpaint=inpaint[, seeded_noise=True]);
    ``prepare(seeds, t_start)`` puts the stacked initial latents in place (edit_prepare_fn); engine.denoise(None, ...).
    step_noise as in two_stage_fns; with "seed" the step noise rows read are the schedule's rows t_start .. (the device step counter), as
    in the pipelines' ``step_noise="seeded"`` call with one generator per sample."""
    return _stage_fns(engine, scheduler, preview_steps, final_steps, step_noise, schedule_kw, strength, prepare, inpaint)


def pair_groups():
    """one process group per (rank r, rank r + 1 mod W) pair, created collectively (every rank calls this once, same order): the
    communicators of the CFG-split final denoise.  Returns {owner: (group, helper)}; {} at world 1."""
    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    out = {}
    if world < 2:
        return out
    for r in range(world):
        h = (r + 1) % world
        out[r] = (dist.new_group(ranks=sorted((r, h))), h)
    return out


def pair_exchange(group, role):
    """exchange(mine) -> (uncond, cond) for DenoiseEngine.denoise_cfg_split: one all_gather of this rank's half of the noise
    prediction inside the pair's group (group rank 0 holds the unconditional half).  gloo cannot move device tensors of every dtype:
    there the halves travel through host memory (tests); RCCL gathers in place over xGMI."""
    def exchange(mine):
        if dist.get_backend(group) == "gloo" and mine.device.type != "cpu":
            halves = [torch.empty(mine.shape, dtype=torch.float32) for _ in range(2)]
            dist.all_gather(halves, mine.detach().float().cpu(), group=group)
            return halves[0].to(mine.device, mine.dtype), halves[1].to(mine.device, mine.dtype)
        halves = [torch.empty_like(mine) for _ in range(2)]
        dist.all_gather(halves, mine.contiguous(), group=group)
        return halves[0], halves[1]
    assert role in (0, 1)
    return exchange


def run_pns(denoise_fn: Callable[[torch.Tensor], torch.Tensor], seeds: Sequence[int], latent_shape,
            scorer: Callable[[torch.Tensor], torch.Tensor] = default_scorer, device="cpu",
            final_fn: Optional[Callable[[torch.Tensor], torch.Tensor]] = None, batch: int = 1,
            final_split_fn: Optional[Callable] = None, pairs=None, pass_seeds: bool = False):
    """Each rank runs ``denoise_fn(noise [S,4,h,w]) -> latents [S,4,h,w]`` for its share of ``seeds`` (the preview,
    or the full denoise when ``final_fn`` is None), scores them, and the group agrees on the winner.
    ``batch`` = candidates per denoise call (S <= batch): with N > world seeds a rank stacks its candidates into one
    UNet batch (BASELINE.json configs[4]: 4 per GPU -> UNet batch 8), 1.2-1.3x the images/sec of one at a time on
    MI355X; candidates stay independent, so the scores do not depend on ``batch``.

    ``final_split_fn(noise, exchange, role) -> latents`` + ``pairs`` (pair_groups()): the final denoise of the winner is shared
    by its owner rank and the next rank -- each computes one half of the CFG pair per step and ``exchange`` swaps them
    (DenoiseEngine.denoise_cfg_split) -- so the serial tail of the two-stage schedule runs on half-size UNet batches; the other
    ranks idle at the winner broadcast as before.  Falls back to ``final_fn`` at world 1.

    ``pass_seeds=True``: ``denoise_fn``, ``final_fn`` and ``final_split_fn`` are also given ``seeds=<the seeds of the candidates in the
    call, in stacking order>`` as a keyword, for functions that derive the per-step noise of a stochastic sampler from the candidate
    seed (two_stage_fns(step_noise="seed")).  The default calls them exactly as before.

    Returns dict(best_seed, best_score, scores [N], latents = the winner's latents on every rank;
    with ``final_fn`` the winner's noise is re-denoised by its owner rank and that result is returned)."""
    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    rank = dist.get_rank() if world > 1 else 0
    seeds = list(seeds)
    mine = shard(seeds, rank, world)
    per = (len(seeds) + world - 1) // world
    local_scores = torch.full((per,), float("-inf"), dtype=torch.float32, device=device)
    local_lat = {}
    for j0 in range(0, len(mine), max(1, int(batch))):
        group = mine[j0:j0 + max(1, int(batch))]
        lat = denoise_fn(torch.cat([seed_latents(s, latent_shape) for s in group], 0), **(dict(seeds=list(group)) if pass_seeds else {}))
        sc = scorer(lat)
        for k, s in enumerate(group):
            local_scores[j0 + k] = sc[k].to(device)
            local_lat[s] = lat[k:k + 1].detach().clone()
    if world > 1:
        gathered = [torch.empty_like(local_scores) for _ in range(world)]
        dist.all_gather(gathered, local_scores)
    else:
        gathered = [local_scores]
    scores = torch.full((len(seeds),), float("-inf"), dtype=torch.float32)
    for r in range(world):
        for j, _ in enumerate(shard(seeds, r, world)):
            scores[j * world + r] = gathered[r][j].item()
    best = int(torch.argmax(scores))            # ties -> lowest index: identical on every rank
    owner = best % world
    best_seed = seeds[best]
    skw = dict(seeds=[best_seed]) if pass_seeds else {}
    split = final_split_fn is not None and pairs and world > 1
    helper = pairs[owner][1] if split else None
    if split and rank in (owner, helper):
        group = pairs[owner][0]
        role = sorted((owner, helper)).index(rank)          # group rank 0 = the unconditional half
        out = final_split_fn(seed_latents(best_seed, latent_shape), pair_exchange(group, role), role, **skw).detach().clone()
        out = out.to(device=device, dtype=torch.float32).contiguous()
    elif rank == owner:
        out = local_lat[best_seed]
        if final_fn is not None:
            out = final_fn(seed_latents(best_seed, latent_shape), **skw).detach().clone()
        out = out.to(device=device, dtype=torch.float32).contiguous()
    else:
        out = torch.empty((1,) + tuple(latent_shape[1:]), dtype=torch.float32, device=device)
    if world > 1:
        dist.broadcast(out, src=owner)
    return dict(best_seed=best_seed, best_score=float(scores[best]), scores=scores, latents=out, owner=owner)
