"""Execution context: maps torch tensors (device memory + streams only -- plumbing) onto the
C ABI of libimh_hip.so, either eagerly (one ctypes call per op) or by RECORDING the calls into a
C++ plan that is later replayed / captured into a hipGraph (one UNet forward is ~1000 launches;
issuing them from Python would cost more than the GPU time).

Nothing here computes with torch: tensors are allocated, viewed and handed over as raw pointers.
"""
import ctypes as C
import json
import os

import torch

from . import lib as L

_DT = {torch.bfloat16: L.IMH_DT_BF16, torch.float16: L.IMH_DT_F16}
_TUNING_PATH = os.environ.get("IMH_TUNING_PATH") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuning.json")   # override: A/B runs


_TUNING_CACHE = None


def _load_tuning():
    """parsed once per process (every eager processor call builds a Ctx)"""
    global _TUNING_CACHE
    if _TUNING_CACHE is None:
        _TUNING_CACHE = _read_tuning()
    return _TUNING_CACHE


def _read_tuning():
    try:
        with open(_TUNING_PATH) as f:
            raw = json.load(f)
        extra = os.environ.get("IMH_TUNING_OVERRIDE")      # A/B aid: a JSON object of entries laid over tuning.json, e.g. '{"2048,10240,1280,0,1": [23256, 160, 1]}'
        if extra:
            raw.update(json.loads(extra))
        return {tuple(int(v) for v in k.split(",")): tuple(cfg) for k, cfg in raw.items()}
    except (OSError, ValueError):
        return {}


# Upsample2D = nearest x2 + conv3x3(pad 1): of the nine taps of output pixel (2y + py, 2x + px) several read the SAME low-res pixel, so every
# output phase (py, px) is a 2 x 2-tap conv on the low-res input whose weights are sums of the 3 x 3 ones -- rows: py = 0: a = 0 -> ky 0,
# a = 1 -> ky 1 + 2; py = 1: a = 0 -> ky 0 + 1, a = 1 -> ky 2 (columns alike), tap (a, b) at low-res pixel (y + py - 1 + a, x + px - 1 + b),
# zero outside the low-res image
_PHASE_TAPS = (((0,), (1, 2)), ((0, 1), (2,)))


def phase_pack(w4):
    """[Cout, Cin, 3, 3] -> the phase-packed weight [4 * Cout, 4 * Cin] of Ctx.conv3x3(up=2), fp32: row block p = 2 * py + px, K order
    (a, b, cin); every entry the fp32 sum of the 1, 2 or 4 taps it stands for (the caller rounds ONCE to the model dtype)"""
    w4 = w4.detach().float()
    Cout, Cin = w4.shape[:2]
    out = w4.new_empty(4, Cout, 2, 2, Cin)
    for py in range(2):
        for px in range(2):
            for a in range(2):
                for b in range(2):
                    acc = None
                    for ky in _PHASE_TAPS[py][a]:
                        for kx in _PHASE_TAPS[px][b]:
                            acc = w4[:, :, ky, kx] if acc is None else acc + w4[:, :, ky, kx]
                    out[2 * py + px, :, a, b, :] = acc
    return out.reshape(4 * Cout, 4 * Cin)


class GnStats:
    """GroupNorm partials of ONE tensor (csrc/imh_lnstats.h gn_emit / norm.hip gn_stats_kernel): t [B, nblk, C / sub, 2] fp32 =
    (sum, M2) per (sample, pixel block, sub-run of `sub` channels); npart = elements per partial (0: the ragged blocks of the
    stand-alone statistics kernel).  Travels with the tensor from the launch that wrote it to every GroupNorm that reads it
    (directly or through a channel concat)."""
    __slots__ = ("t", "nblk", "sub", "npart", "C")

    def __init__(self, t, nblk, sub, npart, C_):
        self.t, self.nblk, self.sub, self.npart, self.C = t, int(nblk), int(sub), int(npart), int(C_)


class GnSpec:
    """A GroupNorm as its consumer's prologue sees it (round 5): the statistics of the input (one GnStats, or two for a channel concat),
    gamma / beta, groups, eps -- the consuming launch builds the (scale, shift) table of its sample itself (imh_gemm_args.gn_part /
    IMH_GN_TABLE_APPLY) instead of reading one written by a table launch."""
    def __init__(self, stats, gamma, beta, groups, eps):
        self.srcs = list(stats) if isinstance(stats, (list, tuple)) else [stats]
        self.gamma, self.beta, self.groups, self.eps = gamma, beta, int(groups), float(eps)
        self.C = sum(g.C for g in self.srcs)

    def check(self, B, Cc, descr):
        if not 1 <= len(self.srcs) <= 2 or self.C != Cc:
            raise L.ImhError(f"{descr}: statistics of {self.C} channels from {len(self.srcs)} source(s) do not fit C={Cc}")
        cpg = Cc // self.groups
        for g in self.srcs:
            if tuple(g.t.shape) != (B, g.nblk, g.C // g.sub, 2) or g.t.dtype != torch.float32 or cpg % g.sub or self.srcs[0].C % g.sub:
                raise L.ImhError(f"{descr}: statistics {tuple(g.t.shape)} (sub {g.sub}) do not fit C={Cc}, groups={self.groups}")

    def tensors(self):
        return tuple(g.t for g in self.srcs) + (self.gamma, self.beta)


class Ctx:
    def __init__(self, device, dtype=torch.bfloat16, record=False, dry=False):
        """dry=True (record only): tensors may live on the CPU; the plan can be inspected (op list,
        FLOP / byte accounting) but never run -- used by the host-logic tests, not a compute path."""
        self.lib = L.load()
        self.device = torch.device(device)
        self.dry = bool(dry and record)
        if self.device.type != "cuda" and not self.dry:
            raise L.ImhError("imagharmony_amd needs a ROCm device (there is no CPU path)")
        if dtype not in _DT:
            raise L.ImhError(f"unsupported compute dtype {dtype}")
        self.dtype = dtype
        self.dt = _DT[dtype]
        self.record = record
        self.plan = self.lib.imh_plan_create() if record else None
        self.keep = []          # tensors referenced by recorded ops
        self.tag = 0
        self.tags = []          # per recorded op: (tag, kind, descr, flops, bytes, shape, epilogue/config dict)
        self._pool = {}
        self._bases = {}        # storage ptr -> pool-owned base tensor
        self._live = set()
        self._ws = None
        self.tuning = _load_tuning()
        # XCD cell shape every GEMM / implicit-GEMM launch of this context asks for (imh_gemm_args.xcd: 0 = the byte-count model,
        # 2 .. 5 = 8 x 1 / 4 x 2 / 2 x 4 / 1 x 8 cells over M x N; + 10: the GEGLU launches (N = 8 C) keep the model's N-major
        # choice); placement only -- DenoiseEngine measures which one this box prefers
        self.xcd_cells = 0
        self.captured = False
        self._ops = []          # recorded (kind, ctypes args, cold tensors) for the weight-prefetch pass
        self._pf_done = False
        self._zero_slabs = {}

    # ------------------------------------------------------------------ memory
    def new(self, *shape, dtype=None):
        dtype = dtype or self.dtype
        n = 1
        for s in shape:
            n *= int(s)
        nb = n * torch.empty((), dtype=dtype).element_size()
        key = (nb + 255) // 256 * 256
        lst = self._pool.get(key)
        if lst:
            base = lst.pop()
        else:
            base = torch.empty(key, dtype=torch.uint8, device=self.device)
            self._bases[base.data_ptr()] = base
            if self.record:
                self.keep.append(base)
        self._live.add(base.data_ptr())
        return base[:nb].view(dtype).view(*shape)

    def free(self, t):
        """Return an activation buffer (or any view of it) to the pool.  Only legal once every op
        that reads it has been emitted (stream order makes later reuse safe)."""
        ptr = t.untyped_storage().data_ptr()
        base = self._bases.get(ptr)
        if base is None:
            return                      # not pool-owned (weights, caller tensors)
        if ptr not in self._live:
            raise L.ImhError("Ctx.free: buffer freed twice")
        self._live.discard(ptr)
        self._pool.setdefault(base.numel(), []).append(base)

    def zeros(self, *shape, dtype=None):
        t = torch.zeros(*shape, dtype=dtype or self.dtype, device=self.device)
        if self.record:
            self.keep.append(t)
        return t

    def zero_slab(self, *shape):
        """a zero-initialised buffer shared by every caller that asks for this shape: for ops that write only part of it and need the
        rest to stay zero (the padded token rows of a ragged self-attention); its users run in stream order, like the pool's"""
        t = self._zero_slabs.get(shape)
        if t is None:
            t = self._zero_slabs[shape] = self.zeros(*shape)
        return t

    def workspace(self, nbytes):
        if self._ws is None or self._ws.numel() < nbytes:
            # (a recording context keeps one generous slab for the whole plan; an eager context -- one per conditioning-module call --
            # takes what the launch needs: 64 MB per call was a device allocation per Resampler pass)
            floor = (64 << 20) if self.record else (1 << 20)
            self._ws = torch.empty(max((int(nbytes) + (1 << 20) - 1) >> 20 << 20, floor), dtype=torch.uint8, device=self.device)
            if self.record:
                self.keep.append(self._ws)
        return self._ws

    def stream(self):
        if self.dry:
            raise L.ImhError("a dry-run context cannot execute (no CPU path)")
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ------------------------------------------------------------------ emit
    def _emit(self, kind, args, ew_op=0, descr="", flops=0.0, nbytes=0.0, keep=(), shape=None, epi=None, free=()):
        """the one way a launch leaves Python: recorded into the plan, or handed to the eager entry point L.OPS names for its kind.
        free: pool buffers that only this launch reads (the statistics of _ln_stats) -- returned once it is emitted"""
        if self.record:
            if kind == L.OP_GEMM and not self.dry:
                # a launch the library refuses is refused HERE, not when the plan first runs (imh_plan_add copies the arguments unseen)
                L.check(self.lib.imh_gemm_check(C.byref(args)), descr or "gemm")
            rc = self.lib.imh_plan_add(self.plan, kind, C.byref(args), ew_op, self.tag)
            if rc < 0:
                L.check(rc, "imh_plan_add")
            self.keep.extend(k for k in keep if k is not None)
            # (a two-problem launch is tagged as the GEMMs it computes; its _ops row keeps the plan kind, which finalize_prefetch reads)
            self.tags.append((self.tag, L.OP_GEMM if kind == L.OP_GEMM_DUAL else kind, descr, flops, nbytes, shape, epi))
            self._ops.append((kind, args, self._cold(keep) if kind in (L.OP_GEMM, L.OP_GEMM_DUAL, L.OP_XATTN, L.OP_XATTN_REGIONS) else []))
        else:
            _, entry, call = L.OPS[kind]
            L.check(call(getattr(self.lib, entry), args, ew_op, self.stream()), descr or f"op kind {kind}")
        for t in free:
            self.free(t)

    @staticmethod
    def _p(t):
        return None if t is None else t.data_ptr()

    def _chk(self, t, name, dtype=None):
        if t is None:
            return
        if t.device != self.device and not (t.device.type == "cuda" and t.device.index == (self.device.index or 0)):
            raise L.ImhError(f"{name}: tensor on {t.device}, context on {self.device}")
        if t.dtype != (dtype or self.dtype):
            raise L.ImhError(f"{name}: dtype {t.dtype}, expected {dtype or self.dtype}")

    # ------------------------------------------------------------------ GEMM / conv
    # variant codes (include/imh.h): what each family can do, so that a tuning-table entry (keyed by shape only) is never
    # handed a launch it rejects
    _WS = (1464, 2464, 24128, 23256, 22128)   # wave-specialised (gemm_ring.hip); 22128: two workgroups per CU
    _W16 = (26256,)                           # sixteen-wave 256 x 320 (gemm_w16.hip): row-form folded LayerNorm (+ GEGLU) launches only
    _PP = (8256, 9128, 9256)                  # ping-pong (gemm_pp.hip)
    _HALO = (7128, 7564, 7328, 7428, 7256, 7356)   # LDS-halo conv3x3, stride 1 (7328 / 7428: weight rings; 7256 / 7356: 16 x 16 patch)

    _PHASE = ((1464, 160), (2464, 160), (24128, 160), (23256, 160), (23256, 128), (5258, 320))   # tiles that run the phase form (conv3x3 up=2)

    @classmethod
    def _variant_ok(cls, bm, sp, flags, conv, stride, ln_pre, M=0, N=0, extras=False, pad=0):
        """extras: the launch has a bias, residual, row-add, second token source (x2) or transposed store (yt) -- the epilogue inputs the
        sixteen-wave tile has none of (gemm_w16_launch refuses them, and whole tiles only); x2 and yt narrow the choice further in gemm()
        itself (plain / wave-specialised tiles; _yt_config); pad: the conv padding mode
        (imh_gemm_args.pad -- 1, right / bottom only, runs on every conv-capable variant except the LDS-halo kernels)"""
        plain = bm <= 128
        if pad and (not conv or bm in cls._HALO + cls._PP + cls._W16):
            return False
        if bm in cls._W16:
            return not conv and sp == 1 and bool(flags & L.GF_LN_ROW) and not flags & ~(L.GF_LN_ROW | L.GF_GEGLU) and bool(ln_pre) \
                and not extras and M % 256 == 0 and N % 320 == 0
        if bm in cls._HALO:
            return bool(conv) and stride == 1 and not flags & (L.GF_LN_ROW | L.GF_LN_COL | L.GF_VT_PERM)
        if flags & (L.GF_VT_PERM | L.GF_LN_COL):
            return plain and (sp == 1 or not flags & L.GF_LN_COL)
        if flags & L.GF_LN_ROW:
            return sp == 1 and not conv and (plain or bm in cls._WS)
        if bm in cls._PP and conv:
            return False
        return True

    def _xcd_for(self, N, flags, conv):
        """imh_gemm_args.xcd of one launch under this context's policy (xcd_cells): 0 / 2..5 = the same request for every launch;
        1x = x for every launch except the GEGLU ones (model).  (A policy that asked for whole-row cells only on the Linear launches
        with small weights -- N <= 1280 -- measured no different from the model on two boxes where 4 x 2 / 8 x 1 EVERYWHERE were 0.2-1.0
        ms ahead: profiles/r04_forward_ab_xcd_policies_box*.json; dropped.)"""
        pol, cells = divmod(self.xcd_cells, 10)
        if pol == 1 and flags & L.GF_GEGLU:
            return 0
        return cells

    def _config(self, M, N, K, conv, flags, stride=1, ln_pre=False, up=0, extras=False, pad=0):
        """tile variant of a launch: the tuning table's entry for the shape if that variant implements the launch's flags
        (folded LayerNorm in either form, V^T permutation, conv stride), else the built-in heuristic -- in ONE place"""
        key = (M, N, K, int(conv))
        # a fifth key field: 1 = the entry for launches whose LayerNorm statistics are precomputed (other variants apply);
        # 2 = the entry for a stride-2 conv whose (M, N, K) coincides with a stride-1 conv of another resolution / batch;
        # 3 = the entry for a conv with fused x2 upsampling (round 6: the 64^2 -> 128^2 upsampler of UNet batch 2 shares (M, N, K) with the
        # 64^2 ResBlock convs of UNet batch 8, which want the LDS-halo form that fuses their GroupNorm);
        # 4 = the phase form of an upsampler conv (conv3x3 up=2; keyed by ITS GEMM: M = B H W low-res pixels, N = 4 Cout, K = 4 Cin; conv_up_phase_cfg)
        cfg = (self.tuning.get(key + (1,)) if ln_pre else self.tuning.get(key + (2,)) if conv and stride == 2
               else self.tuning.get(key + (3,)) if conv and up else None) or self.tuning.get(key)
        if cfg is not None and self._variant_ok(cfg[0], cfg[2], flags, conv, stride, ln_pre, M, N, extras, pad):
            return tuple(cfg)
        bm, bn, sp = C.c_int(), C.c_int(), C.c_int()
        self.lib.imh_gemm_pick_config(M, N, K, C.byref(bm), C.byref(bn), C.byref(sp))
        bm, bn, sp = bm.value, bn.value, sp.value
        if flags & (L.GF_LN_ROW | L.GF_LN_COL) and (sp > 1 or cfg is not None):
            # the statistics need the whole K range in one workgroup; a rejected table entry means a small-tile problem
            bm, bn, sp = (128, 128, 1) if M * N >= 8192 * 640 else (64, 64, 1)
        return bm, bn, sp

    def gemm(self, x, w, out=None, bias=None, residual=None, rowadd=None, rows_per_batch=0, ldra=0, flags=0,
             M=None, N=None, K=None, ldx=None, ldw=None, ldy=None, ldr=None, cfg=None, descr="gemm", out_dtype=None,
             ln=None, stats_out=False, gn_out=None, x2=None, yt=None, _args_only=False):
        """y[M, N] = epilogue(x[M, K] @ w[N, K]^T).  x / w: 2-D, last dim contiguous.
        ln = (s, c, eps[, stats]) with GF_LN_ROW / GF_LN_COL in flags: LayerNorm of the token operand folded into the GEMM
        (w pre-scaled by gamma); stats = (tensor [tokens, slots, 2] fp32, slots) are the token rows' statistics as handed
        over by the launch that wrote them (csrc/imh_lnstats.h); None -> a row-statistics launch over the token rows
        supplies them (the kernels have no in-loop E[x^2] - mean^2 form).
        stats_out=True: also return the row statistics of y for a LayerNorm-folding consumer -> (y, (tensor, slots)); they
        come from the GEMM's own epilogue when the chosen variant has one, else from a row-statistics launch over y.
        gn_out=hw (rows per sample; a (groups, hw) pair is accepted, the groups are the consumer's business): y is a GroupNorm
        input -> (y, gn) with gn = GnStats from the epilogue, or None when the chosen variant has no such epilogue (the consumer
        then runs gn_stats over y).
        yt = (Yt [N - col0, ldyt], col0): output columns >= col0 are stored transposed in the V^T layout into Yt instead of y (y
        then holds columns [0, col0)); wave-specialised bn = 160 variants and 23256 x 128, flags == GF_LN_ROW only, whole tiles, no
        residual / row-add (the one-launch [Q|K|V]); without cfg= a table entry or heuristic tile that cannot do it gives way to the first
        such variant that tiles M, N and col0 (_yt_config), and where none does the call raises here.
        x2: the token operand is the column concat [x | x2] (K = x.shape[1] + x2.shape[1]; the up blocks' conv_shortcut over
        torch.cat([hidden, skip], 1)) read from its two producers -- plain 64 / 128 tiles (split-K included) and the wave-specialised
        variants; without cfg= any other table entry gives way to a plain tile.
        In a recording context the library's launch checks run at this call (imh_gemm_check), so a refusal never waits for the replay."""
        self._chk(x, descr + ".x"); self._chk(w, descr + ".w")
        M = M if M is not None else x.shape[0]
        K = K if K is not None else x.shape[1] + (x2.shape[1] if x2 is not None else 0)
        N = N if N is not None else w.shape[0]
        if x.stride(-1) != 1 or w.stride(-1) != 1:
            raise L.ImhError(f"{descr}: operands must be contiguous in K")
        if x2 is not None:
            self._chk(x2, descr + ".x2")
            if x2.shape[0] != x.shape[0] or x2.stride(-1) != 1 or x.shape[1] % 64 or x2.shape[1] % 64 or x.shape[1] + x2.shape[1] != K \
                    or x2.stride(0) != x2.shape[1] or (flags & (L.GF_LN_ROW | L.GF_LN_COL | L.GF_VT_PERM)):
                raise L.ImhError(f"{descr}: x2 must be a dense [M, K2] block with K1, K2 multiples of 64 and K1 + K2 == K (no folded LayerNorm)")
        if isinstance(gn_out, tuple):
            gn_out = gn_out[1]
        n_out = N // 2 if flags & L.GF_GEGLU else N
        if yt is not None:
            n_out = int(yt[1])
        if out is None:
            out = self.new(M, n_out, dtype=torch.float32 if flags & L.GF_OUT_F32 else None)
        ln_stats, own = None, ()
        if ln is not None:
            fold = flags & (L.GF_LN_ROW | L.GF_LN_COL)
            ln_stats, own = self._ln_stats(ln, (lambda: (x[:M, :K] if flags & L.GF_LN_ROW else w[:N, :K])) if fold and not _args_only else None, descr)
            if fold and ln_stats is None:
                raise L.ImhError(f"{descr}: a folded-LayerNorm problem of gemm_dual needs its row statistics (gemm_dual supplies them)")
        if stats_out and flags & L.GF_OUT_F32:
            raise L.ImhError(f"{descr}: stats_out describes rows stored in the compute dtype; an fp32 output (GF_OUT_F32) has no such statistics")
        if stats_out and gn_out is not None:
            raise L.ImhError(f"{descr}: stats_out and gn_out are mutually exclusive (one consumer norm per output)")
        bm, bn, sp = cfg or self._config(M, N, K, 0, flags, ln_pre=ln_stats is not None, extras=any(
            t is not None for t in (bias, residual, rowadd, x2, yt)))
        if yt is not None:
            bm, bn, sp = self._yt_config(M, N, int(yt[1]), flags, (bm, bn, sp), cfg is not None, residual is not None or rowadd is not None, descr)
        if x2 is not None and not (bm <= 128 or bm in self._WS):
            if cfg is not None:
                raise L.ImhError(f"{descr}: variant {bm} does not read a two-source token operand")
            bm, bn, sp = (128, 128, 1) if M * N >= 8192 * 640 else (64, 64, 1)
        if _args_only:
            sp = 1
        a = self._gemm_args(x, w, out, (M, N, K), (ldx if ldx is not None else x.stride(0), ldw if ldw is not None else w.stride(0),
                                                   ldy if ldy is not None else out.stride(0)), (bm, bn, sp), flags=flags,
                            bias=bias, rowadd=rowadd, residual=residual, ldra=ldra, rows_per_batch=rows_per_batch, x2=x2,
                            ldr=(ldr if ldr is not None else residual.stride(0)) if residual is not None else 0)
        if yt is not None:
            self._chk(yt[0], descr + ".yt")
            if yt[0].dim() != 2 or yt[0].stride(1) != 1 or yt[0].shape[0] != N - int(yt[1]) or yt[0].shape[1] < M:
                raise L.ImhError(f"{descr}: yt {tuple(yt[0].shape)} does not fit [{N - int(yt[1])}, >= {M}]")
            a.Yt, a.yt_col0, a.ldyt = yt[0].data_ptr(), int(yt[1]), yt[0].stride(0)
        keep_ln = self._ln_fold(a, ln, ln_stats)           # (s, c fp32, eps[, stats]); the caller sets GF_LN_ROW / GF_LN_COL in flags
        es = x.element_size()
        keep = (x, w, out, bias, rowadd, residual, x2) + keep_ln
        if _args_only:
            return a, out, 2.0 * M * N * K, es * (M * K + N * K + M * n_out), keep
        st = None
        if stats_out:
            wd = self.lib.imh_gemm_stats_slot_width(bm, bn)
            # (a folded-LayerNorm launch of a wave-specialised variant ends in the lean epilogue, which emits none: gemm_launch refuses)
            if wd > 0 and N % wd == 0 and sp == 1 and not flags & (L.GF_GEGLU | L.GF_VT_PERM | L.GF_OUT_F32) \
                    and not (bm > 128 and flags & (L.GF_LN_ROW | L.GF_LN_COL)):
                st = (self.new(M, N // wd, 2, dtype=torch.float32), N // wd)
                a.ln_stats_out, a.ln_slots_out = st[0].data_ptr(), st[1]
        gn = self._gn_epilogue(a, gn_out) if gn_out is not None else None
        self._emit(L.OP_GEMM, a, descr=descr, flops=2.0 * M * N * K, nbytes=es * (M * K + N * K + M * n_out),
                   keep=keep + ((st[0],) if st else ()) + ((gn.t,) if gn else ()) + ((yt[0],) if yt is not None else ()),
                   shape=(M, N, K, 0, None), free=own,
                   epi=self._gemm_epi(a, gn, gn_out, ln_pre=ln_stats is not None, ln_slots=int(ln_stats[1]) if ln_stats is not None else 0,
                                      stats_out=st is not None, yt=int(yt[1]) if yt is not None else 0))
        if stats_out:
            if st is None:
                st = self.row_stats(out.view(M, n_out) if out.dim() != 2 else out, descr=descr + ".row_stats")
            return out, st
        if gn_out is not None:
            return out, gn
        return out

    def _gemm_args(self, x, w, out, mnk, ld, cfg, flags=0, geom=None, bias=None, rowadd=None, residual=None, ldr=0, ldra=0, rows_per_batch=0,
                   x2=None):
        """the L.GemmArgs of every GEMM and implicit-GEMM launch: operands, mnk = (M, N, K), ld = (ldx, ldw, ldy), cfg = (bm, bn, splits)
        with the split-K workspace, the XCD request; geom = (H, W, Cin, Ho, Wo, stride, up, pad) makes it a conv3x3.  x2: the second
        token / channel source, read after the x.shape[-1] columns of x"""
        a = L.GemmArgs()
        a.X, a.W, a.Y = x.data_ptr(), w.data_ptr(), out.data_ptr()
        a.bias, a.rowadd, a.residual = self._p(bias), self._p(rowadd), self._p(residual)
        if x2 is not None:
            a.X2, a.Cin1 = x2.data_ptr(), x.shape[-1]
        a.M, a.N, a.K = mnk
        a.ldx, a.ldw, a.ldy = ld
        a.ldr, a.ldra, a.rows_per_batch = ldr, ldra, rows_per_batch
        a.bm, a.bn, a.splits = cfg
        a.flags, a.dtype, a.conv = flags, self.dt, int(geom is not None)
        a.xcd = self._xcd_for(a.N, flags, a.conv)
        if geom is not None:
            a.H, a.Wd, a.Cin, a.Ho, a.Wo, a.stride, a.up, a.pad = geom
        if a.splits > 1:
            a.partial = self.workspace(self.lib.imh_gemm_workspace_bytes(a.M, a.N, a.splits)).data_ptr()
        return a

    @staticmethod
    def _gemm_epi(a, gn, gn_hw, **more):
        """the epilogue / config dict of a GEMM or conv3x3 launch as ctx.tags keeps it; gn = the GnStats its epilogue writes (or None) over
        gn_hw rows per sample"""
        return dict(flags=a.flags, bias=bool(a.bias), residual=bool(a.residual), rowadd=bool(a.rowadd), rows_per_batch=a.rows_per_batch,
                    cfg=(a.bm, a.bn, a.splits), gn_out=(gn.nblk, gn_hw) if gn else None, x2=a.Cin1 if a.X2 else 0, **more)

    def _ln_stats(self, ln, rows, descr):
        """the statistics of a folded LayerNorm ln = (s, c, eps[, stats]), for every launch that folds one: those the caller hands over,
        else those of a row-statistics launch over the token rows rows() -- its buffer goes back to the pool once the consumer is emitted
        (_emit(free=...)).  rows=None: no launch.  -> ((tensor, slots) or None, buffers to free)"""
        if len(ln) > 3 and ln[3] is not None:
            return ln[3], ()
        if rows is None:
            return None, ()
        st = self.row_stats(rows(), descr=descr + ".ln_row_stats")
        return st, (st[0],)

    def _ln_fold(self, a, ln, stats):
        """ln = (s, c, eps[, ...]) and its statistics into the ln_* fields GemmArgs and the fused cross-attentions share -> tensors to keep"""
        if ln is None:
            return ()
        a.ln_s, a.ln_c, a.ln_eps = ln[0].data_ptr(), ln[1].data_ptr(), float(ln[2])
        if stats is None:
            return ln[0], ln[1]
        a.ln_stats, a.ln_slots = stats[0].data_ptr(), int(stats[1])
        return ln[0], ln[1], stats[0]

    # (bm, bn, tile rows) that carry the transposed store (gemm_launch: every wave-specialised variant at bn = 160, and 23256 x 128)
    _YT = ((23256, 160, 256), (24128, 160, 128), (2464, 160, 64), (1464, 160, 64), (23256, 128, 256), (22128, 160, 128))

    def _yt_config(self, M, N, col0, flags, c, forced, extra, descr):
        """tile variant of a yt= launch (gemm_launch's rule for imh_gemm_args.Yt): a wave-specialised bn = 160 variant or 23256 x 128, flags ==
        GF_LN_ROW only, no residual / row-add / split-K, whole tiles, 0 < col0 < N a multiple of bn.  c = what the table / heuristic (or the
        caller: forced) chose; when that is not such a variant the first of _YT the library builds that tiles M, N and col0 serves"""
        if flags != L.GF_LN_ROW or extra or not 0 < col0 < N:
            raise L.ImhError(f"{descr}: Yt (the transposed V^T store, yt=) needs flags == GF_LN_ROW only, no residual / row-add and 0 < col0 < N "
                             f"(flags={flags}, col0={col0}, N={N})")
        fits = lambda bm, bn, rows: M % rows == 0 and N % bn == 0 and col0 % bn == 0
        for bm, bn, rows in self._YT:
            if (bm, bn) == tuple(c[:2]) and c[2] == 1 and fits(bm, bn, rows):
                return c
        if not forced:
            for bm, bn, rows in self._YT:
                if L.variant_built((bm, bn)) and fits(bm, bn, rows):
                    return bm, bn, 1
        raise L.ImhError(f"{descr}: Yt (the transposed V^T store, yt=) needs a wave-specialised bn = 160 variant or 23256 x 128 with whole tiles and col0 a "
                         f"multiple of bn (variant {tuple(c)}, M={M}, N={N}, col0={col0})")

    def _gn_epilogue(self, a, hw, phases=1):
        """GroupNorm partials from the launch's epilogue (imh_gemm_args.gn_out) if its variant and shape have one: fills the
        fields of a and returns the GnStats of the output ([B, blocks, N / 10, 2] fp32), else None.  hw: rows of a per sample.
        phases = 4: the phase form of conv3x3(up=2), whose N is four phases of N / 4 output channels -- one partial per (sample, `rows`
        consecutive low-res pixels, phase, 10 channels): block ph * (hw / rows) + low-res row block"""
        rows = self.lib.imh_gemm_gn_block_rows(a.bm, a.bn)
        halo = a.bm in self._HALO
        N = a.N // phases
        if (rows <= 0 or a.splits != 1 or N % 10 or hw % rows or a.M % hw
                or N % (a.bn if halo else 80) or a.flags & ~(L.GF_ACT_SILU | L.GF_ACT_GELU | L.GF_ACT_QGELU)
                or (halo and (a.Ho % (rows // 4) or a.Wo % 16))):
            return None
        nblk = phases * (hw // rows)
        t = self.new(a.M // hw, nblk, N // 10, 2, dtype=torch.float32)
        a.gn_out, a.gn_nblk, a.gn_hw = t.data_ptr(), nblk, hw
        return GnStats(t, nblk, 10, rows * 10, N)

    def row_stats(self, x, descr="row_stats"):
        """LayerNorm statistics of token rows x [rows, C] in the hand-over format (one slot per row): the stand-alone
        producer for rows whose writing GEMM variant has no statistics epilogue"""
        rows, Cc = x.shape
        st = self.new(rows, 1, 2, dtype=torch.float32)
        self.ew(L.EW_ROW_STATS, st, a=x, n=rows, i=(Cc, x.stride(0), 0, 0, 0, 0), descr=descr,
                nbytes=float(x.numel() * x.element_size()))
        return st, 1

    def gemm_dual(self, g1, g2, cfg=(128, 64), descr="gemm_dual"):
        """Two independent GEMMs (dicts of gemm() keyword arguments incl. x, w) in one launch.  The folded-LayerNorm pair
        (g1 row form on x, g2 column form with the same token rows as its w) shares one statistics tensor; when the caller has
        none, a row-statistics launch over the token rows supplies it."""
        for g in (g1, g2):
            if g.get("x2") is not None or g.get("yt") is not None or g.get("gn_out") is not None or g.get("stats_out"):
                raise L.ImhError(f"{descr}: x2 / yt / gn_out / stats_out are single-problem (Ctx.gemm) features")
        own = ()
        l1, l2 = g1.get("ln"), g2.get("ln")
        if l1 is not None:
            st, own = self._ln_stats(l1, lambda: g1["x"], descr)
            if own:
                g1 = dict(g1, ln=tuple(l1[:3]) + (st,))
                if l2 is not None and (len(l2) < 4 or l2[3] is None):
                    g2 = dict(g2, ln=tuple(l2[:3]) + (st,))
        a1, o1, f1, b1, k1 = self.gemm(_args_only=True, cfg=(cfg[0], cfg[1], 1), **g1)
        a2, o2, f2, b2, k2 = self.gemm(_args_only=True, cfg=(cfg[0], cfg[1], 1), **g2)
        # (keep: the cold-weight candidates, _cold's first two, are those of k1[:2] + k2[:2])
        self._emit(L.OP_GEMM_DUAL, (L.GemmArgs * 2)(a1, a2), descr=descr, flops=f1 + f2, nbytes=b1 + b2, keep=k1[:2] + k2[:2] + k1[2:] + k2[2:],
                   free=own, epi=dict(dual=((a1.M, a1.N, a1.K, a1.flags), (a2.M, a2.N, a2.K, a2.flags)), cfg=tuple(cfg),
                                      ln_pre=bool(a1.ln_stats), ln_slots=int(a1.ln_slots)))
        return o1, o2

    def conv_fuses_gn(self, M, N, K, stride=1, up=0, cfg=None):
        """True when the conv3x3 launch of this shape runs on the LDS-halo kernel, which takes the GroupNorm (+ SiLU) of its input
        (gn=...) and a two-source channel concat (x2=...) in its halo staging"""
        bm, bn, sp = cfg or self._config(M, N, K, 1, 0, stride=stride, up=up)
        if bm not in self._HALO or stride != 1 or up:
            return False
        # the table of the front end ([Cin][2] fp32) shares the workgroup's LDS with the halo buffers and the weight ring, whose depth differs
        # between the kernel families and with the A/B mode (imh_debug_set key 5): the launcher's own byte count, not a copy of it
        lds = self.lib.imh_conv_halo_lds_bytes(bm, bn, K // 9, 1)
        return 0 < lds <= 160 * 1024

    def conv_up_phase_cfg(self, B, H, W, Cin, Cout, cfg=None):
        """tile variant (bm, bn, 1) of the phase form of an upsampler conv (conv3x3 up=2) over a [B, H, W, Cin] input, or None when the
        launch does not qualify (the caller then runs the up=1 form): a column tile must lie inside one phase (Cout % bn == 0) on a variant
        that carries the phase gather and store; imh_debug_set(11, 0) switches the form off (A/B)"""
        if Cin % 64 or Cout % 8 or min(B, H, W) < 1 or self.lib.imh_debug_set(11, -1) != 1:
            return None
        c = cfg or self.tuning.get((B * H * W, 4 * Cout, 4 * Cin, 1, 4)) or ((23256, 160, 1) if Cout % 160 == 0 else (23256, 128, 1))
        bm, bn, sp = c
        if (bm, bn) not in self._PHASE or Cout % bn or sp != 1:
            return None
        return bm, bn, 1

    def _conv3x3_phase(self, x, w, w_phase, bias, out, cfg, descr, gn_groups):
        """conv3x3(up=2): the conv behind a nearest x2 upsampling as four 2 x 2-tap phase convs on the LOW-res input in one implicit GEMM --
        M = B H W, N = 4 Cout (phase-major), K = 4 Cin: 4/9 of the multiply-adds of the up=1 form"""
        B, H, W, Cin = x.shape
        if w_phase is None:       # one-off callers (tests): pack from the [Cout, 9 Cin] weight here; models cache theirs (unet.Conv2d.packed_phase)
            self._chk(w, descr + ".w")
            if w.dim() != 2 or w.shape[1] != 9 * Cin:
                raise L.ImhError(f"{descr}: w must be packed [Cout, 9*Cin]")
            w_phase = phase_pack(w.view(w.shape[0], 3, 3, Cin).permute(0, 3, 1, 2)).to(self.dtype).contiguous()
        self._chk(x, descr + ".x"); self._chk(w_phase, descr + ".w_phase")
        Cout = w_phase.shape[0] // 4
        if not x.is_contiguous() or not w_phase.is_contiguous() or tuple(w_phase.shape) != (4 * Cout, 4 * Cin):
            raise L.ImhError(f"{descr}: x must be contiguous NHWC and w_phase [4*Cout, 4*Cin]")
        c = self.conv_up_phase_cfg(B, H, W, Cin, Cout, cfg=cfg)
        if c is None:
            raise L.ImhError(f"{descr}: the phase form (up=2) does not run this launch (Cin {Cin} % 64, Cout {Cout} % tile width, variant "
                             f"{cfg}, imh_debug_set key 11); use up=1 (Ctx.conv_up_phase_cfg)")
        Ho, Wo = 2 * H, 2 * W
        M, N, K = B * H * W, 4 * Cout, 4 * Cin
        if out is None:
            out = self.new(B, Ho, Wo, Cout)
        a = self._gemm_args(x, w_phase, out, (M, N, K), (Cin, K, Cout), c, geom=(H, W, Cin, Ho, Wo, 1, 2, 0), bias=bias, rows_per_batch=H * W)
        gs = self._gn_epilogue(a, H * W, phases=4) if gn_groups else None
        es = x.element_size()
        # (recorded as the conv it computes -- output pixels x Cout x 9 Cin, geometry up = 2, the conv's algorithmic FLOPs like every other
        # launch; the launch executes 4/9 of them, 2 M N K)
        self._emit(L.OP_GEMM, a, descr=descr, flops=2.0 * (B * Ho * Wo) * Cout * 9 * Cin, nbytes=es * (M * Cin + N * K + 4 * M * Cout),
                   keep=(x, w_phase, out, bias) + ((gs.t,) if gs else ()),
                   shape=(B * Ho * Wo, Cout, 9 * Cin, 1, (B, H, W, Cin, 1, 2)),
                   epi=dict(self._gemm_epi(a, gs, Ho * Wo, gn_in=None), rows_per_batch=Ho * Wo))
        return (out, gs) if gn_groups else out

    def conv3x3(self, x, w, bias=None, stride=1, up=0, residual=None, rowadd=None, ldra=0, out=None, cfg=None,
                descr="conv3x3", gn_groups=0, gn=None, x2=None, pad=0, w_phase=None):
        """x: NHWC [B, H, W, Cin]; w: packed [Cout, 9*Cin]; returns NHWC [B, Ho, Wo, Cout]; with gn_groups > 0 (the output is
        a GroupNorm input) -> (y, GnStats or None) as gemm(gn_out=...).
        gn = (table [B, Cin, 2] fp32 from gn_table(), silu) or (GnSpec, silu): the input's GroupNorm (+ SiLU) is applied inside the
        kernel's halo staging (diffusers ResnetBlock2D: norm -> nonlinearity -> conv in one launch) -- with a GnSpec the kernel also builds
        the table itself from the producers' partials (no table launch); x2: the input is the channel concat [x | x2].  Both need the
        LDS-halo variant (conv_fuses_gn).
        pad = 1: no padding on the top / left, one zero pixel on the right / bottom (diffusers Downsample2D(padding=0), the VAE
        encoder's downsamplers; stride 2): Ho = (H - 2) // 2 + 1.
        up = 2: the same result as up = 1 (nearest x2 upsampling, then the conv) computed in the phase form (_conv3x3_phase; w_phase =
        phase_pack() of the weight in the model dtype, packed here from w when None); bias only, raises when the launch does not qualify
        (conv_up_phase_cfg)."""
        if up == 2:
            if stride != 1 or pad or residual is not None or rowadd is not None or gn is not None or x2 is not None:
                raise L.ImhError(f"{descr}: the phase form (up=2) is a plain stride-1 conv with a bias (no residual, row-add, fused GroupNorm or second source)")
            return self._conv3x3_phase(x, w, w_phase, bias, out, cfg, descr, gn_groups)
        self._chk(x, descr + ".x"); self._chk(w, descr + ".w")
        B, H, W, C1 = x.shape
        Cin = C1 + (x2.shape[-1] if x2 is not None else 0)
        Cout = w.shape[0]
        Hv, Wv = H << up, W << up
        if pad and (stride != 2 or up or gn is not None or x2 is not None):
            raise L.ImhError(f"{descr}: pad mode 1 is a plain stride-2 conv (no upsampling, fused GroupNorm or second source)")
        Ho, Wo = ((Hv - 2) // 2 + 1, (Wv - 2) // 2 + 1) if pad else ((Hv - 1) // stride + 1, (Wv - 1) // stride + 1)
        M, N, K = B * Ho * Wo, Cout, 9 * Cin
        if not x.is_contiguous() or not w.is_contiguous() or w.shape[1] != K:
            raise L.ImhError(f"{descr}: x must be contiguous NHWC and w packed [Cout, 9*Cin]")
        if x2 is not None:
            self._chk(x2, descr + ".x2")
            if tuple(x2.shape[:3]) != (B, H, W) or not x2.is_contiguous() or C1 % 64 or x2.shape[-1] % 64:
                raise L.ImhError(f"{descr}: x2 must be contiguous NHWC over the same pixels, both channel counts multiples of 64")
        if out is None:
            out = self.new(B, Ho, Wo, Cout)
        # (the table is keyed by (M, N, K): a stride-2 conv can share its key with a stride-1 conv of another resolution /
        # batch; the LDS-halo kernel is stride-1 only -> _config falls back to the heuristic tile for that one)
        bm, bn, sp = cfg or self._config(M, N, K, 1, 0, stride=stride, up=up, pad=pad)
        if (gn is not None or x2 is not None) and not self.conv_fuses_gn(M, N, K, stride, up, cfg=(bm, bn, sp)):
            raise L.ImhError(f"{descr}: the fused GroupNorm front end / two-source input need the LDS-halo conv3x3 (variant {bm} x {bn}, "
                             f"stride {stride}, up {up}); apply the GroupNorm / concat as passes for this launch (Ctx.conv_fuses_gn)")
        a = self._gemm_args(x, w, out, (M, N, K), (Cin, K, Cout), (bm, bn, sp), geom=(H, W, Cin, Ho, Wo, stride, up, pad), bias=bias, rowadd=rowadd,
                            residual=residual, ldr=Cout if residual is not None else 0, ldra=ldra, rows_per_batch=Ho * Wo, x2=x2)
        gn_keep = ()
        if gn is not None and isinstance(gn[0], GnSpec):
            sp_, silu = gn
            sp_.check(B, Cin, descr)
            self._gn_sources(a, sp_.srcs)
            a.gn_gamma, a.gn_beta, a.gn_groups, a.gn_eps, a.gn_silu = self._p(sp_.gamma), self._p(sp_.beta), sp_.groups, sp_.eps, int(bool(silu))
            gn_keep = sp_.tensors()
        elif gn is not None:
            tab, silu = gn
            if tuple(tab.shape) != (B, Cin, 2) or tab.dtype != torch.float32 or not tab.is_contiguous():
                raise L.ImhError(f"{descr}: GroupNorm table {tuple(tab.shape)} does not fit [{B}, {Cin}, 2] fp32")
            a.gn_tab, a.gn_silu = tab.data_ptr(), int(bool(silu))
            gn_keep = (tab,)
        gs = self._gn_epilogue(a, Ho * Wo) if gn_groups else None
        es = x.element_size()
        self._emit(L.OP_GEMM, a, descr=descr, flops=2.0 * M * N * K,
                   nbytes=es * (B * H * W * Cin + N * K + M * N),
                   keep=(x, w, out, bias, rowadd, residual, x2) + ((gs.t,) if gs else ()) + gn_keep,
                   shape=(M, N, K, 1, (B, H, W, Cin, stride, up) + ((pad,) if pad else ())),
                   epi=self._gemm_epi(a, gs, Ho * Wo, gn_in=None if gn is None else int(bool(gn[1]))))
        return (out, gs) if gn_groups else out

    # the fields that take the first of one or two GnStats (partials, blocks, sub-run width, elements per partial, channels) in the argument
    # structs that read GroupNorm partials; the second source's are these names + "2", and it has no channel count of its own
    _GN_SRC = {L.GemmArgs: ("gn_part", "gn_pnblk", "gn_psub", "gn_pnpart", "gn_pC1"), L.NormArgs: ("partial", "nblk", "sub", "npart", "C1")}

    @classmethod
    def _gn_sources(cls, a, srcs):
        """one or two GnStats (a channel concat [a | b]) into the source fields of a conv3x3 / gn_table / gn_table_apply launch"""
        for sfx, g in zip(("", "2"), srcs):
            for name, v in zip(cls._GN_SRC[type(a)][:4 if sfx else 5], (g.t.data_ptr(), g.nblk, g.sub, g.npart, g.C)):
                setattr(a, name + sfx, v)

    # ------------------------------------------------------------------ attention
    def attention(self, q, k, vt, out, B, H, Lq, Lk, Lk_pad, ldq, ldk, ldvt, ldo, scale,
                  k2=None, vt2=None, Lk2=0, Lk2_pad=0, ldk2=0, ldvt2=0, scale2=0.0, scale2_tab=None, step=None,
                  descr="attention"):
        a = self._attn_args(L.AttnArgs(), out, B, H, Lq, (k, vt, Lk, Lk_pad, ldk, ldvt), (k2, vt2, Lk2, Lk2_pad, ldk2, ldvt2), ldo,
                            (scale, scale2, scale2_tab, step))
        a.Q, a.ldq = q.data_ptr(), ldq
        es = q.element_size()
        fl = 4.0 * B * H * Lq * (Lk + Lk2) * 64
        by = es * (2 * B * Lq * H * 64 + 2 * B * (Lk + Lk2) * H * 64)
        self._emit(L.OP_ATTN, a, descr=descr, flops=fl, nbytes=by, keep=(q, k, vt, out, k2, vt2, scale2_tab, step),
                   shape=(B, H, Lq, Lk, Lk_pad), epi=dict(Lk2=Lk2, Lk2_pad=Lk2_pad, tab=scale2_tab is not None))
        return out

    def _attn_args(self, a, out, B, H, Lq, keys, keys2, ldo, scales):
        """what AttnArgs, XAttnArgs and XAttnRegionsArgs share: keys = (k, vt, Lk, Lk_pad, ldk, ldvt), keys2 the same of the second key
        set (tensors None / zeros without one), scales = (scale, scale2, scale2_tab, step)"""
        (k, vt, a.Lk, a.Lk_pad, a.ldk, a.ldvt), (k2, vt2, a.Lk2, a.Lk2_pad, a.ldk2, a.ldvt2) = keys, keys2
        a.K, a.Vt, a.K2, a.Vt2, a.O = k.data_ptr(), vt.data_ptr(), self._p(k2), self._p(vt2), out.data_ptr()
        a.B, a.H, a.Lq, a.ldo, a.dtype = B, H, Lq, ldo, self.dt
        a.scale, a.scale2, tab, step = scales
        a.scale2_tab, a.step = self._p(tab), self._p(step)
        return a

    def _xattn_args(self, a, x, wq, out, B, H, Lq, keys, keys2, scales, ln, descr):
        """XAttnArgs / XAttnRegionsArgs: _attn_args plus the fused to_q's x / wq / folded LayerNorm with the statistics the CALLER handed
        over (the launch's own come from _ln_stats) -> (a, those statistics or None)"""
        self._chk(x, descr + ".x"); self._chk(wq, descr + ".wq")
        C_ = H * 64
        if x.shape[-1] != C_ or tuple(wq.shape) != (C_, C_) or x.stride(-1) != 1 or wq.stride(-1) != 1:
            raise L.ImhError(f"{descr}: x [.., {C_}] / wq [{C_}, {C_}] expected, got {tuple(x.shape)} / {tuple(wq.shape)}")
        self._attn_args(a, out, B, H, Lq, keys, keys2, out.stride(0), scales)
        a.X, a.Wq, a.C, a.ldx, a.ldw = x.data_ptr(), wq.data_ptr(), C_, x.stride(0), wq.stride(0)
        st = self._ln_stats(ln, None, descr)[0] if ln is not None else None
        self._ln_fold(a, ln, st)
        return a, st

    def _emit_xattn(self, kind, a, ln, st, own, keep, fl, by, descr, **epi):
        """the tag row both fused cross-attentions share"""
        self._emit(kind, a, descr=descr, flops=fl, nbytes=by, keep=keep + tuple((ln or ())[:2]) + ((st[0],) if st is not None else ()),
                   shape=(a.B, a.H, a.Lq, a.Lk, a.Lk_pad), free=own,
                   epi=dict(Lk2=a.Lk2, Lk2_pad=a.Lk2_pad, tab=bool(a.scale2_tab), ln=ln is not None, ln_slots=int(a.ln_slots) if ln is not None else 0, **epi))

    def cross_attention(self, x, wq, k, vt, out, B, H, Lq, Lk, Lk_pad, ldk, ldvt, scale, ln=None,
                        k2=None, vt2=None, Lk2=0, Lk2_pad=0, ldk2=0, ldvt2=0, scale2=0.0, scale2_tab=None, step=None,
                        descr="cross.fused"):
        """out[B*Lq, C] = attention(to_q(LN?(x)), K, V) (+ scale2 * attention(., K2, V2)) in one launch
        (csrc/xattn.hip).  x [B*Lq, C]; wq [C, C]; k / k2 caches with head dims in vt_perm16 order (GF_VT_PERM);
        ln = (s, c, eps[, stats]): x is un-normalised and wq pre-scaled by gamma; stats as in gemm() (None -> a row-statistics
        launch over x supplies them)."""
        a, st = self._xattn_args(L.XAttnArgs(), x, wq, out, B, H, Lq, (k, vt, Lk, Lk_pad, ldk, ldvt), (k2, vt2, Lk2, Lk2_pad, ldk2, ldvt2),
                                 (scale, scale2, scale2_tab, step), ln, descr)
        own = ()
        if ln is not None and st is None:
            st, own = self._ln_stats(ln, lambda: x.view(-1, a.C), descr)
            self._ln_fold(a, ln, st)
        es = x.element_size()
        M, C_ = B * Lq, a.C
        fl = 2.0 * M * C_ * C_ + 4.0 * B * H * Lq * (Lk + Lk2) * 64
        by = es * (2 * M * C_ + C_ * C_ + 2 * B * (Lk + Lk2) * C_)
        self._emit_xattn(L.OP_XATTN, a, ln, st, own, (x, wq, k, vt, out, k2, vt2, scale2_tab, step), fl, by, descr)
        return out

    @staticmethod
    def regions_refusal(a):
        """the argument rules of imh_cross_attention_regions (csrc/api.hip do_xattn_regions, csrc/xattn_regions.hip xattn_regions_launch)
        restated over a filled L.XAttnRegionsArgs: None when the library launches it, else the reason.  imh_plan_add copies a launch's
        arguments unseen, so the recorder refuses HERE what the library would refuse when the plan first runs."""
        if not (a.X and a.Wq and a.K and a.Vt and a.K2 and a.Vt2 and a.O and a.mask):
            return "null pointer argument"
        if bool(a.ln_s) != bool(a.ln_c) or (a.ln_s and not a.ln_eps > 0.0):
            return "folded LayerNorm needs ln_s, ln_c and ln_eps > 0"
        if ((a.mask or 0) | (a.weights or 0)) & 3:
            return "mask and weights must be 4-byte aligned"
        if bool(a.scale2_tab) != bool(a.step):
            return "scale2_tab and step come together"
        if a.C != a.H * 64:
            return f"C={a.C} must be H*64 (H={a.H})"
        if a.ln_s and not a.ln_stats:
            return "the folded LayerNorm takes the token rows' statistics from ln_stats"
        if a.ln_s and (a.ln_slots <= 0 or a.C % a.ln_slots):
            return f"ln_slots={a.ln_slots} must divide C={a.C}"
        if not 1 <= a.n_img <= L.REGIONS_MAX_IMAGES:
            return f"n_img={a.n_img} must be 1 .. {L.REGIONS_MAX_IMAGES}"
        if a.Lk <= 0 or a.Lk_pad % 64 or a.Lk_pad < a.Lk:
            return f"Lk={a.Lk} Lk_pad={a.Lk_pad} (pad must be a multiple of 64 and >= Lk)"
        if a.Lk2 <= 0 or a.Lk2_pad % 64 or a.Lk2_pad < a.Lk2:
            return f"Lk2={a.Lk2} Lk2_pad={a.Lk2_pad} invalid"
        if a.C <= 0 or a.C % 64:
            return f"C={a.C} must be a positive multiple of 64"
        if any(int(v) & 7 for v in (a.ldx, a.ldw, a.ldk, a.ldvt, a.ldo, a.ldk2, a.ldvt2)):
            return "leading dimensions must be multiples of 8 elements"
        if a.B <= 0 or a.H <= 0 or a.Lq <= 0:
            return "empty problem"
        if a.ldm < a.Lq:
            return f"ldm={a.ldm} is shorter than a mask row of Lq={a.Lq} values"
        if a.dtype not in (L.IMH_DT_BF16, L.IMH_DT_F16):
            return f"unknown dtype {a.dtype}"
        return None

    def cross_attention_regions(self, x, wq, k, vt, out, B, H, Lq, Lk, Lk_pad, ldk, ldvt, scale, k2, vt2, Lk2, Lk2_pad, ldk2, ldvt2,
                                n_img, mask, weights=None, ln=None, scale2=1.0, scale2_tab=None, step=None, descr="cross.regions"):
        """cross_attention() with n_img masked image prompts per sample in one launch (csrc/xattn_regions.hip, include/imh_regions.h):
        out = attention(to_q(LN?(x)), K, V) + sum_i (g * weights[i]) * mask[i, q] * attention(., K2_i, V2_i), g = scale2_tab[*step] or
        scale2.  k2 / vt2 hold image i of batch b at key (b * n_img + i) * Lk2_pad (the K / V projection of the image tokens as a batch of
        B * n_img); mask fp32 [n_img, >= Lq] (rows mask.stride(0) apart), weights fp32 [n_img] or None (all 1), both on the device.
        What the library refuses is refused here, where the launch is recorded."""
        self._chk(mask, descr + ".mask", torch.float32); self._chk(weights, descr + ".weights", torch.float32)
        self._chk(scale2_tab, descr + ".scale2_tab", torch.float32); self._chk(step, descr + ".step", torch.int32)
        if mask is None or k2 is None or vt2 is None:
            raise L.ImhError(f"{descr}: k2, vt2 and mask are required")
        a, st = self._xattn_args(L.XAttnRegionsArgs(), x, wq, out, B, H, Lq, (k, vt, Lk, Lk_pad, ldk, ldvt), (k2, vt2, Lk2, Lk2_pad, ldk2, ldvt2),
                                 (scale, scale2, scale2_tab, step), ln, descr)
        C_ = a.C
        n_img = int(n_img)
        if mask.dim() != 2 or mask.stride(1) != 1 or mask.shape[0] != n_img or mask.shape[1] < Lq:
            raise L.ImhError(f"{descr}: mask {tuple(mask.shape)} must be fp32 [n_img = {n_img}, >= Lq = {Lq}] with unit column stride")
        if weights is not None and (weights.dim() != 1 or weights.numel() != n_img or not weights.is_contiguous()):
            raise L.ImhError(f"{descr}: weights {tuple(weights.shape)} must be a dense fp32 vector of n_img = {n_img}")
        keys2 = B * n_img * Lk2_pad
        if k2.dim() != 2 or vt2.dim() != 2 or k2.shape[0] < keys2 or vt2.shape[1] < keys2 or k2.shape[1] < C_ or vt2.shape[0] < C_:
            raise L.ImhError(f"{descr}: k2 {tuple(k2.shape)} / vt2 {tuple(vt2.shape)} do not hold B * n_img * Lk2_pad = {keys2} keys of {C_} dims")
        a.n_img, a.mask, a.ldm, a.weights = n_img, mask.data_ptr(), mask.stride(0), self._p(weights)
        need, own = ln is not None and st is None, ()
        if need:
            a.ln_stats, a.ln_slots = 1, 1           # (row_stats' one slot per row, a placeholder pointer: the statistics launch comes after the rule check)
        why = self.regions_refusal(a)
        if why:
            raise L.ImhError(f"{descr}: {why}")
        if need:
            st, own = self._ln_stats(ln, lambda: x.view(-1, C_), descr)
            self._ln_fold(a, ln, st)
        es = x.element_size()
        M = B * Lq
        fl = 2.0 * M * C_ * C_ + 4.0 * B * H * Lq * (Lk + n_img * Lk2) * 64
        by = es * (2 * M * C_ + C_ * C_ + 2 * B * (Lk + n_img * Lk2) * C_) + 4.0 * n_img * Lq
        self._emit_xattn(L.OP_XATTN_REGIONS, a, ln, st, own, (x, wq, k, vt, out, k2, vt2, scale2_tab, step, mask, weights), fl, by, descr, n_img=n_img)
        return out

    # ------------------------------------------------------------------ fp32 (reference-precision) ops of the VAE decode tail (csrc/f32.hip)
    def _f32(self, op, a, descr):
        if self.record:
            raise L.ImhError(f"{descr}: the fp32 ops run eagerly (once per image); they are not plan ops")
        L.check(self.lib.imh_f32(op, C.byref(a), self.stream()), descr)

    def f32_gemm(self, x, w, bias=None, residual=None, out=None, M=None, N=None, K=None, ldx=None, ldw=None, descr="f32.gemm"):
        """y[M, N] = x[M, K] @ w[N, K]^T (+ bias) (+ residual), everything fp32 (v_mfma_f32_32x32x2_f32); K % 16 == 0"""
        for t, n in ((x, "x"), (w, "w"), (bias, "bias"), (residual, "residual"), (out, "out")):
            self._chk(t, f"{descr}.{n}", torch.float32)
        M = M if M is not None else x.shape[0]
        K = K if K is not None else x.shape[1]
        N = N if N is not None else w.shape[0]
        if out is None:
            out = self.new(M, N, dtype=torch.float32)
        a = L.F32Args()
        a.X, a.W, a.Y, a.bias, a.residual = x.data_ptr(), w.data_ptr(), out.data_ptr(), self._p(bias), self._p(residual)
        a.M, a.N, a.K = M, N, K
        a.ldx = ldx if ldx is not None else x.stride(0)
        a.ldw = ldw if ldw is not None else w.stride(0)
        a.ldy = out.stride(0)
        a.ldr = residual.stride(0) if residual is not None else 0
        self._f32(L.F32_GEMM, a, descr)
        return out

    def f32_conv3x3(self, x, w, bias=None, residual=None, up=0, stride=1, pad=0, descr="f32.conv3x3"):
        """x NHWC [B, H, W, Cin] fp32, w packed [Cout, 9 Cin] fp32 -> [B, Ho, Wo, Cout]: stride 1 with padding 1 and optional nearest x2
        (Ho = H << up), or stride 2 with padding 1 (Ho = (H - 1) // 2 + 1) or, pad = 1, right / bottom only (Ho = (H - 2) // 2 + 1)"""
        for t, n in ((x, "x"), (w, "w"), (bias, "bias"), (residual, "residual")):
            self._chk(t, f"{descr}.{n}", torch.float32)
        B, H, W, Cin = x.shape
        Cout = w.shape[0]
        if stride == 1:
            Ho, Wo = H << up, W << up
        else:
            Ho, Wo = ((H - 2) // 2 + 1, (W - 2) // 2 + 1) if pad else ((H - 1) // 2 + 1, (W - 1) // 2 + 1)
        if not x.is_contiguous() or not w.is_contiguous() or w.shape[1] != 9 * Cin:
            raise L.ImhError(f"{descr}: x must be contiguous NHWC and w packed [Cout, 9*Cin]")
        out = self.new(B, Ho, Wo, Cout, dtype=torch.float32)
        a = L.F32Args()
        a.X, a.W, a.Y, a.bias, a.residual = x.data_ptr(), w.data_ptr(), out.data_ptr(), self._p(bias), self._p(residual)
        a.M, a.N, a.K = B * Ho * Wo, Cout, 9 * Cin
        a.ldx, a.ldw, a.ldy, a.ldr = Cin, 9 * Cin, Cout, (residual.stride(-2) if residual is not None else 0)
        a.conv, a.H, a.Wd, a.Cin, a.Ho, a.Wo, a.up, a.stride, a.pad = 1, H, W, Cin, Ho, Wo, up, stride, pad
        self._f32(L.F32_GEMM, a, descr)
        return out

    def img2img_init(self, out, moments, n1, n2, scaling, add_a, add_b, descr="img2img.init"):
        """out [S, 4, h, w] fp32 = add_a * scaling * (mean + exp(0.5 clamp(logvar, -30, 20)) * n1) + add_b * n2 in one launch
        (diffusers' posterior sample + scaling_factor + scheduler.add_noise); moments [M, h, w, 8] fp32 NHWC (the quant_conv output),
        n1 [N, 4, h, w], n2 [S, 4, h, w]; sample s reads moments s % M and posterior noise s % N"""
        for t, n in ((out, "out"), (moments, "moments"), (n1, "n1"), (n2, "n2")):
            self._chk(t, f"{descr}.{n}", torch.float32)
            if not t.is_contiguous():
                raise L.ImhError(f"{descr}: {n} must be contiguous")
        S, c4, h, w = out.shape
        M, N = moments.shape[0], n1.shape[0]
        if c4 != 4 or tuple(moments.shape[1:]) != (h, w, 8) or tuple(n1.shape[1:]) != (4, h, w) or tuple(n2.shape) != (S, 4, h, w):
            raise L.ImhError(f"{descr}: shapes out {tuple(out.shape)} moments {tuple(moments.shape)} n1 {tuple(n1.shape)} n2 {tuple(n2.shape)}")
        a = L.F32Args()
        a.X, a.W, a.Y, a.residual = moments.data_ptr(), n1.data_ptr(), out.data_ptr(), n2.data_ptr()
        a.B, a.HW, a.M, a.N = S, h * w, M, N
        a.scale, a.add_a, a.add_b = float(scaling), float(add_a), float(add_b)
        self._f32(L.F32_IMG2IMG_INIT, a, descr)
        return out

    def f32_groupnorm(self, x, gamma, beta, groups, eps, silu=False, descr="f32.groupnorm"):
        """x [B, HW, C] fp32 -> GroupNorm(groups)(+ SiLU), fp32; statistics as shifted (sum, M2) partials merged in double"""
        for t, n in ((x, "x"), (gamma, "gamma"), (beta, "beta")):
            self._chk(t, f"{descr}.{n}", torch.float32)
        B, HW, Cc = x.shape
        nblk = max(1, (HW + 2047) // 2048)
        part = self.new(B, nblk, groups, 2, dtype=torch.float32)
        tab = self.new(B, Cc, 2, dtype=torch.float32)
        y = self.new(B, HW, Cc, dtype=torch.float32)
        a = L.F32Args()
        a.X, a.ws, a.B, a.HW, a.C, a.groups, a.nblk, a.eps, a.silu = x.data_ptr(), part.data_ptr(), B, HW, Cc, groups, nblk, float(eps), int(silu)
        self._f32(L.F32_GN_STATS, a, descr + ".stats")
        a.gamma, a.beta, a.Y = gamma.data_ptr(), beta.data_ptr(), tab.data_ptr()
        self._f32(L.F32_GN_TABLE, a, descr + ".table")
        a.ws, a.Y = tab.data_ptr(), y.data_ptr()
        self._f32(L.F32_GN_APPLY, a, descr + ".apply")
        self.free(part); self.free(tab)
        return y

    def f32_softmax(self, a_, out, scale, descr="f32.softmax"):
        """out[r, :] = softmax(scale * a_[r, :]), fp32 rows"""
        self._chk(a_, descr + ".a", torch.float32); self._chk(out, descr + ".out", torch.float32)
        a = L.F32Args()
        a.X, a.Y, a.M, a.N, a.ldx, a.ldy, a.scale = a_.data_ptr(), out.data_ptr(), a_.shape[0], a_.shape[1], a_.stride(0), out.stride(0), float(scale)
        self._f32(L.F32_SOFTMAX, a, descr)
        return out

    def attention_small(self, q, k, v, B, H, Lq, Lk, dq, dv, scale, out=None, descr="attention_small"):
        """q [B*Lq, H*dq], k [B*Lk, H*dq], v [B*Lk, H*dv] row-major (any row stride) -> [B*Lq, H*dv]"""
        if out is None:
            out = self.new(B * Lq, H * dv)
        a = L.SmallAttnArgs()
        a.Q, a.K, a.V, a.O = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
        a.B, a.H, a.Lq, a.Lk, a.dq, a.dv = B, H, Lq, Lk, dq, dv
        a.ldq, a.ldk, a.ldv, a.ldo = q.stride(0), k.stride(0), v.stride(0), out.stride(0)
        a.scale, a.dtype = scale, self.dt
        self._emit(L.OP_ATTN_SMALL, a, descr=descr, flops=2.0 * B * H * Lq * Lk * (dq + dv), keep=(q, k, v, out))
        return out

    def attention_enc(self, q, k, v, B, H, L_, d, scale=None, out=None, descr="attention_enc", causal=False):
        """encoder attention with a generic head dim (imh_attention_enc; causal=True: imh_attention_enc_causal, query q sees keys <= q):
        q, k, v [B*L, >= H*d] row-major with any row stride -- e.g. the three column ranges of one packed QKV GEMM output -- -> [B*L, H*d]"""
        for t, nm in ((q, "q"), (k, "k"), (v, "v")):
            self._chk(t, f"{descr}.{nm}")
            if t.dim() != 2 or t.stride(1) != 1 or t.shape[0] != B * L_ or t.shape[1] < H * d:
                raise L.ImhError(f"{descr}: {nm} {tuple(t.shape)} must be row-major [{B * L_}, >= {H * d}]")
        if out is None:
            out = self.new(B * L_, H * d)
        self._chk(out, descr + ".out")
        if out.dim() != 2 or out.stride(1) != 1 or out.shape[0] != B * L_ or out.shape[1] < H * d:
            raise L.ImhError(f"{descr}: out {tuple(out.shape)} must be row-major [{B * L_}, >= {H * d}]")
        a = L.EncAttnArgs()
        a.Q, a.K, a.V, a.O = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
        a.B, a.H, a.L, a.d = B, H, L_, d
        a.ldq, a.ldk, a.ldv, a.ldo = q.stride(0), k.stride(0), v.stride(0), out.stride(0)
        a.scale, a.dtype = float(scale if scale is not None else d ** -0.5), self.dt
        self._emit(L.OP_ATTN_ENC_CAUSAL if causal else L.OP_ATTN_ENC, a, descr=descr, flops=(2.0 if causal else 4.0) * B * H * L_ * L_ * d,
                   nbytes=float(q.element_size()) * 4 * B * L_ * H * d, keep=(q, k, v, out))
        return out

    # ------------------------------------------------------------------ norms
    def _norm_args(self, mode, B, HW, Cc, groups=1, eps=1.0, silu=0, rows=0, **tensors):
        """the L.NormArgs of every GroupNorm pass and of layernorm; tensors: pointer fields by name (None stays null)"""
        a = L.NormArgs()
        a.B, a.HW, a.C, a.groups, a.rows, a.eps, a.silu, a.dtype, a.mode = B, HW, Cc, groups, rows, eps, int(silu), self.dt, mode
        for name, t in tensors.items():
            setattr(a, name, self._p(t))
        return a

    @staticmethod
    def _bhwc(x):
        """(B, HW, C) of a flattened NHWC tensor [B, ..., C]"""
        return x.shape[0], x.numel() // (x.shape[0] * x.shape[-1]), x.shape[-1]

    def gn_stats(self, x, sub=10, descr="gn_stats"):
        """stand-alone GroupNorm statistics of x [B, HW, C] (a pass over x) in the hand-over format -- for tensors whose writing
        launch has no statistics epilogue (conv_in, split-K / ring variants)"""
        self._chk(x, descr + ".x")
        B, HW, Cc = self._bhwc(x)
        if Cc % sub:
            raise L.ImhError(f"{descr}: sub-run width {sub} does not divide C={Cc}")
        nblk = self.lib.imh_groupnorm_stats_blocks(HW, Cc)
        t = self.new(B, nblk, Cc // sub, 2, dtype=torch.float32)
        a = self._norm_args(L.GN_STATS, B, HW, Cc, x=x, partial=t)
        a.sub = sub
        self._emit(L.OP_GROUPNORM, a, descr=descr, nbytes=float(x.numel() * x.element_size()), keep=(x, t))
        return GnStats(t, nblk, sub, 0, Cc)

    def gn_table(self, stats, gamma, beta, groups, eps, HW, descr="gn_table"):
        """(scale, shift) table [B, C, 2] fp32 of a GroupNorm from the partials of its input: stats = GnStats or a list of two
        (channel concat [a | b]: C = a.C + b.C)"""
        spec = GnSpec(stats, gamma, beta, groups, eps)
        B, Cc = (spec.srcs[0].t.shape[0] if spec.srcs else 0), spec.C
        spec.check(B, Cc, descr)
        tab = self.new(B, Cc, 2, dtype=torch.float32)
        a = self._norm_args(L.GN_TABLE, B, HW, Cc, groups, eps, gamma=gamma, beta=beta, table=tab)
        self._gn_sources(a, spec.srcs)
        self._emit(L.OP_GROUPNORM, a, descr=descr, keep=(gamma, beta, tab) + tuple(g.t for g in spec.srcs))
        return tab

    def gn_apply(self, x, tab, silu, out=None, descr="gn_apply"):
        """y = silu?(x * scale + shift) as a pass (the consumers that cannot take the table themselves: Linear layers, the
        implicit-GEMM convs)"""
        self._chk(x, descr + ".x")
        B, HW, Cc = self._bhwc(x)
        if tuple(tab.shape) != (B, Cc, 2) or tab.dtype != torch.float32:
            raise L.ImhError(f"{descr}: table {tuple(tab.shape)} does not fit [{B}, {Cc}, 2]")
        if out is None:
            out = self.new(*x.shape)
        a = self._norm_args(L.GN_APPLY, B, HW, Cc, silu=silu, x=x, y=out, table=tab)
        es = x.element_size()
        self._emit(L.OP_GROUPNORM, a, descr=descr, flops=4.0 * x.numel(), nbytes=2.0 * es * x.numel(), keep=(x, out, tab))
        return out

    def gn_table_apply(self, x, spec, silu, out=None, descr="gn_table_apply"):
        """y = silu?(GroupNorm(x)) in ONE launch from the producers' partials (IMH_GN_TABLE_APPLY): every workgroup of the apply pass
        builds its sample's table in LDS -- the form for consumers that cannot take the norm themselves (Transformer2DModel.norm in
        front of proj_in, conv_norm_out)"""
        self._chk(x, descr + ".x")
        B, HW, Cc = self._bhwc(x)
        spec.check(B, Cc, descr)
        if out is None:
            out = self.new(*x.shape)
        a = self._norm_args(L.GN_TABLE_APPLY, B, HW, Cc, spec.groups, spec.eps, silu, x=x, y=out, gamma=spec.gamma, beta=spec.beta)
        self._gn_sources(a, spec.srcs)
        es = x.element_size()
        self._emit(L.OP_GROUPNORM, a, descr=descr, flops=4.0 * x.numel(), nbytes=2.0 * es * x.numel(), keep=(x, out) + spec.tensors())
        return out

    def groupnorm(self, x, gamma, beta, groups, eps, silu, out=None, descr="groupnorm", stats=None):
        """x: [B, HW, C] (NHWC flattened).  stats = GnStats left by the producing launch's epilogue (gemm(gn_out=...) /
        conv3x3(gn_groups=...)) or by gn_stats(): table + apply, no statistics pass over x; None: statistics + table + apply."""
        self._chk(x, descr + ".x")
        B, HW, Cc = self._bhwc(x)
        if stats is not None:
            if not isinstance(stats, GnStats) or stats.C != Cc or stats.t.shape[0] != B:
                raise L.ImhError(f"{descr}: statistics do not fit x {tuple(x.shape)}")
            return self.gn_table_apply(x, GnSpec(stats, gamma, beta, groups, eps), silu, out=out, descr=descr)
        if out is None:
            out = self.new(*x.shape)
        # scratch use is confined to this op's three kernels (stream order), so the shared workspace is safe
        a = self._norm_args(L.GN_ALL, B, HW, Cc, groups, eps, silu, x=x, y=out, gamma=gamma, beta=beta,
                            partial=self.workspace(self.lib.imh_groupnorm_workspace_bytes(B, HW, Cc, groups)))
        es = x.element_size()
        self._emit(L.OP_GROUPNORM, a, descr=descr, flops=8.0 * x.numel(), nbytes=3.0 * es * x.numel(), keep=(x, out, gamma, beta))
        return out

    def layernorm(self, x, gamma, beta, eps, out=None, descr="layernorm"):
        self._chk(x, descr + ".x")
        Cc = x.shape[-1]
        rows = x.numel() // Cc
        if out is None:
            out = self.new(*x.shape)
        a = self._norm_args(L.GN_ALL, 0, 0, Cc, 0, eps, rows=rows, x=x, y=out, gamma=gamma, beta=beta)      # (mode: unread by imh_layernorm)
        es = x.element_size()
        self._emit(L.OP_LAYERNORM, a, descr=descr, flops=8.0 * x.numel(), nbytes=2.0 * es * x.numel(),
                   keep=(x, out, gamma, beta), shape=(rows, Cc))
        return out

    # ------------------------------------------------------------------ elementwise
    def _chk_dense_f32(self, descr, **named):
        for nm, t in named.items():
            if t is not None:
                self._chk(t, f"{descr}.{nm}", torch.float32)
                if not t.is_contiguous():
                    raise L.ImhError(f"{descr}: {nm} must be contiguous")

    def ew(self, op, y, a=None, b=None, w=None, bias=None, tab=None, step=None, n=0, i=(0, 0, 0, 0, 0, 0),
           f=(0.0, 0.0, 0.0, 0.0), descr="ew", nbytes=0.0, x2=None, noise=None, mask=None, blend_tab=None, hist=None, bank=None,
           seeds=None, noise_stream=0):
        """x2 / noise / mask / blend_tab (fp32, imh.h ABI 11): conv_in's second source, the masked blend behind the CFG step.
        hist / bank (fp32, IMH_EW_CFG_MSTEP only): the history slot the step reads and rewrites in place and the per-step noise bank;
        they travel in the fields `b` and `bias` (imh_ew_args does not grow), so they exclude b= / bias=
        seeds (IMH_EW_CFG_MSTEP only; noise.seed_rows on the device, int32 view of uint32 [S, 4]): the seeded step, imh_step_seeded --
        the step's noise is generated in the launch from the samples' seed rows instead of read from a bank (bank= is then refused)"""
        if seeds is not None:
            if op != L.EW_CFG_MSTEP or bank is not None or bias is not None:
                raise L.ImhError(f"{descr}: seeds belong to EW_CFG_MSTEP and take the place of the noise bank")
            self._chk(seeds, f"{descr}.seeds", torch.int32)
            if tuple(seeds.shape) != (int(i[0]), 4) or not seeds.is_contiguous():
                raise L.ImhError(f"{descr}: seeds {tuple(seeds.shape)} must be a dense [{int(i[0])}, 4] table (noise.seed_rows)")
        if hist is not None or bank is not None:
            if op != L.EW_CFG_MSTEP or b is not None or bias is not None:
                raise L.ImhError(f"{descr}: hist / bank belong to EW_CFG_MSTEP and take the place of b / bias")
            self._chk_dense_f32(descr, hist=hist, bank=bank)
            b, bias = hist, bank
        if op == L.EW_CONCAT and int(i[5]) > 0:
            self._chk_identity_rows(descr, y, b, int(n), i)
        if op in (L.EW_CFG_STEP, L.EW_CFG_MSTEP, L.EW_CFG_RESCALE) and int(i[2]) != 0 and (int(i[2]) != 1 or a is None):
            raise L.ImhError(f"{descr}: i2 = {int(i[2])} selects the three-term (PAG) form with 1 and needs the noise prediction")
        e = L.EwArgs()
        e.a, e.b, e.y, e.w, e.bias = self._p(a), self._p(b), y.data_ptr(), self._p(w), self._p(bias)
        e.tab, e.step = self._p(tab), self._p(step)
        self._chk_dense_f32(descr, x2=x2, noise=noise, mask=mask, blend_tab=blend_tab)
        e.x2, e.noise, e.mask, e.blend_tab = self._p(x2), self._p(noise), self._p(mask), self._p(blend_tab)
        e.n = n
        e.i0, e.i1, e.i2, e.i3, e.i4, e.i5 = i
        e.f0, e.f1, e.f2, e.f3 = f
        e.dtype = self.dt
        if seeds is not None:
            sa = L.SeededArgs()
            sa.ew, sa.seeds, sa.stream = e, seeds.data_ptr(), int(noise_stream)
            self._emit(L.OP_STEP_SEEDED, sa, descr=descr, nbytes=nbytes, keep=(a, b, y, w, tab, step, x2, noise, mask, blend_tab, seeds))
            return y
        self._emit(L.OP_EW, e, ew_op=op, descr=descr, nbytes=nbytes, keep=(a, b, y, w, bias, tab, step, x2, noise, mask, blend_tab))
        return y

    def _chk_identity_rows(self, descr, y, vt, n, i):
        """the identity-attention form of EW_CONCAT (imh.h: i5 = ldvt > 0) is refused here for what the library refuses it for"""
        i0, C_, i2, ldy, col0, ldvt = (int(v) for v in i)
        if i0 != 0 or i2 != 0:
            raise L.ImhError(f"{descr}: the identity-rows form has an empty first part and no FreeU planes (i0 = {i0}, i2 = {i2})")
        if n <= 0 or n % 16 or col0 < 0 or col0 % 16 or C_ <= 0 or C_ % 8:
            raise L.ImhError(f"{descr}: identity rows n = {n}, col0 = {col0} (multiples of 16), C = {C_} (a positive multiple of 8)")
        if ldvt % 8 or ldvt < col0 + n or ldy % 8 or ldy < C_:
            raise L.ImhError(f"{descr}: identity rows ldvt = {ldvt} (a multiple of 8, >= col0 + n = {col0 + n}), ld of y = {ldy} (a multiple of 8, >= C = {C_})")
        if vt is None or vt.data_ptr() % 16 or y.data_ptr() % 16:
            raise L.ImhError(f"{descr}: identity rows need Vt in b, and b and y 16-byte aligned")
        self._chk(vt, f"{descr}.vt"); self._chk(y, f"{descr}.y")

    def identity_rows(self, vt, out, n, col0, descr="identity_rows"):
        """out[r, 0:C] = V[col0 + r, 0:C] for r < n, read from vt = V^T [C, ldvt] as the self-attention projections leave it (keys permuted
        inside every 16-group, imh_layout.h vt_perm16): the attention output of samples whose attention map is the identity
        (perturbed-attention guidance).  The identity-attention form of EW_CONCAT (imh.h: i5 = ldvt > 0), one launch; out: rows of a
        row-major [*, ld] buffer, ld = out.stride(0)."""
        if vt.dim() != 2 or out.dim() != 2 or vt.stride(1) != 1 or out.stride(1) != 1 or out.shape[1] != vt.shape[0] or out.shape[0] < n:
            raise L.ImhError(f"{descr}: V^T {tuple(vt.shape)} and out {tuple(out.shape)} must be row-major [C, ldvt] and [>= n = {n}, C]")
        C_ = int(vt.shape[0])
        return self.ew(L.EW_CONCAT, out, b=vt, n=int(n), i=(0, C_, 0, int(out.stride(0)), int(col0), int(vt.stride(0))), descr=descr,
                       nbytes=2.0 * n * C_ * out.element_size())

    def randn_seeded(self, seeds, HW, row=0, step=None, noise_stream=0, raw=False, out=None, descr="randn_seeded"):
        """the seeded generator's rows by themselves (imh_randn_seeded; imagharmony_amd/noise.py states what they are): fp32 [S, 4, HW]
        normals of (seeds[s], row, noise_stream), or with raw the int32-viewed uint32 words.  seeds: noise.seed_rows on the device
        (int32 [S, 4]); the row is the immediate ``row`` or, with ``step`` (device int32), *step."""
        self._chk(seeds, descr + ".seeds", torch.int32); self._chk(step, descr + ".step", torch.int32)
        if seeds.dim() != 2 or seeds.shape[1] != 4 or not seeds.is_contiguous():
            raise L.ImhError(f"{descr}: seeds {tuple(seeds.shape)} must be a dense [S, 4] table (noise.seed_rows)")
        S, HW = int(seeds.shape[0]), int(HW)
        dt = torch.int32 if raw else torch.float32
        if out is None:
            out = self.new(S, 4, HW, dtype=dt)
        self._chk(out, descr + ".out", dt)
        if tuple(out.shape) != (S, 4, HW) or not out.is_contiguous():
            raise L.ImhError(f"{descr}: out {tuple(out.shape)} must be dense [{S}, 4, {HW}]")
        if not 0 <= int(row) < 2 ** 32:
            raise L.ImhError(f"{descr}: row {row} outside [0, 2**32)")
        a = L.RandnArgs()
        a.y, a.seeds, a.step, a.S, a.HW, a.row, a.stream, a.raw = out.data_ptr(), seeds.data_ptr(), self._p(step), S, HW, int(row), int(noise_stream), int(bool(raw))
        self._emit(L.OP_RANDN_SEEDED, a, descr=descr, nbytes=16.0 * S * HW, keep=(seeds, step, out))
        return out

    def clip_preprocess(self, images, out, size, patch, mean, std, descr="clip_preprocess"):
        """decoded images -> the CLIP tower's patch rows in one launch (imh_clip_preprocess; imagharmony_amd/imageops.py states what they
        are): images fp32 [S, 3, H, W] in [-1, 1], dense; out [S g g, >= 3 patch patch] row-major (any row stride) in bfloat16, float16 or
        float32 -- columns [0, 3 patch patch) of every row are written, the rest of the row is left alone.  The resized extent and the crop
        origin are derived here (imageops.clip_geometry, as ClipPreferenceJudge.preprocess derives them)."""
        from .imageops import clip_geometry
        self._chk(images, descr + ".images", torch.float32)
        if out.dtype not in _DT and out.dtype != torch.float32:
            raise L.ImhError(f"{descr}: out dtype {out.dtype} (bfloat16, float16 or float32)")
        self._chk(out, descr + ".out", out.dtype)
        if images.dim() != 4 or images.shape[1] != 3 or not images.is_contiguous():
            raise L.ImhError(f"{descr}: images {tuple(images.shape)} must be dense [S, 3, H, W]")
        S, _, H, W = (int(v) for v in images.shape)
        size, patch = int(size), int(patch)
        if patch < 1 or size < patch or size % patch:
            raise L.ImhError(f"{descr}: size {size} must be a positive multiple of patch {patch}")
        g, k = size // patch, 3 * patch * patch
        if out.dim() != 2 or out.stride(1) != 1 or out.shape[0] != S * g * g or out.shape[1] < k or out.stride(0) < out.shape[1]:
            raise L.ImhError(f"{descr}: out {tuple(out.shape)} must be row-major [{S * g * g}, >= {k}]")
        nh, nw, top, left = clip_geometry(H, W, size)
        a = L.ClipPreprocessArgs()
        a.x, a.y, a.S, a.H, a.W = images.data_ptr(), out.data_ptr(), S, H, W
        a.nh, a.nw, a.top, a.left, a.size, a.patch, a.ldp = nh, nw, top, left, size, patch, out.stride(0)
        a.mean0, a.mean1, a.mean2 = (float(v) for v in mean)
        a.std0, a.std1, a.std2 = (float(v) for v in std)
        a.dtype = _DT.get(out.dtype, L.CLIP_DT_F32)
        self._emit(L.OP_CLIP_PREPROCESS, a, descr=descr, nbytes=4.0 * images.numel() + float(out.element_size()) * S * g * g * k, keep=(images, out))
        return out

    def control_add(self, x, r, scale=1.0, tab=None, step=None, gn_sub=None, descr="control_add"):
        """y = x + g * r[b % Br] (imh_control_add), g = scale * (tab[*step] if tab is given else 1): the ControlNet's gated residual
        injection.  x [B, ..., C] and r [Br, ..., C] dense NHWC in the compute dtype over the same pixels, B % Br == 0; tab fp32 (device),
        step the device step counter (together or not at all).  The product and the sum are separate fp32 roundings: torch's
        (x.float() + g * r.float()).to(dtype) bit for bit.  Returns a new tensor y shaped like x (there is no in-place form); with
        gn_sub -> (y, GnStats): the GroupNorm partials of y in sub-runs of gn_sub channels from the same launch, bit-equal to
        gn_stats(y, gn_sub).  What the library refuses is refused here, where the launch is recorded."""
        self._chk(x, descr + ".x"); self._chk(r, descr + ".r")
        self._chk(tab, descr + ".tab", torch.float32); self._chk(step, descr + ".step", torch.int32)
        if x.dim() < 2 or r.dim() != x.dim() or not x.is_contiguous() or not r.is_contiguous():
            raise L.ImhError(f"{descr}: x {tuple(x.shape)} / r {tuple(r.shape)} must be dense NHWC tensors of one rank")
        B, Br, Cc = int(x.shape[0]), int(r.shape[0]), int(x.shape[-1])
        if B < 1 or Br < 1 or B % Br or tuple(r.shape[1:]) != tuple(x.shape[1:]) or x.numel() == 0:
            raise L.ImhError(f"{descr}: r {tuple(r.shape)} does not serve x {tuple(x.shape)} (same pixels and channels, a batch that divides B)")
        HW = x.numel() // (B * Cc)
        if Cc % 8 or Cc > 4096 or B > 65535:
            raise L.ImhError(f"{descr}: C={Cc} must be a multiple of 8 up to 4096 (B={B} up to 65535)")
        if (tab is None) != (step is None):
            raise L.ImhError(f"{descr}: tab and step come together")
        if gn_sub is not None and (int(gn_sub) < 1 or Cc % int(gn_sub)):
            raise L.ImhError(f"{descr}: sub-run width {gn_sub} does not divide C={Cc}")
        if not self.dry and (x.data_ptr() | r.data_ptr()) & 15:
            raise L.ImhError(f"{descr}: x and r must be 16-byte aligned")
        y = self.new(*x.shape)
        gs = None
        a = L.ControlAddArgs()
        a.x, a.r, a.y, a.tab, a.step = x.data_ptr(), r.data_ptr(), y.data_ptr(), self._p(tab), self._p(step)
        a.scale, a.B, a.Br, a.HW, a.C, a.dtype = float(scale), B, Br, HW, Cc, self.dt
        if gn_sub is not None:
            nblk = self.lib.imh_groupnorm_stats_blocks(HW, Cc)
            t = self.new(B, nblk, Cc // int(gn_sub), 2, dtype=torch.float32)
            a.partial, a.sub = t.data_ptr(), int(gn_sub)
            gs = GnStats(t, nblk, int(gn_sub), 0, Cc)
        es = x.element_size()
        self._emit(L.OP_CONTROL_ADD, a, descr=descr, flops=2.0 * x.numel(), nbytes=float(es) * (2 * x.numel() + r.numel()),
                   keep=(x, r, y, tab, step) + ((gs.t,) if gs else ()), shape=(B, HW, Cc, Br), epi=dict(tab=tab is not None, gn_sub=gn_sub))
        return (y, gs) if gn_sub is not None else y

    # ------------------------------------------------------------------ T2I-Adapter passes (imh_adapter_op: eager, once per control image)
    def _adapter_op(self, a, descr):
        if self.record:
            raise L.ImhError(f"{descr}: imh_adapter_op is no plan kind: the adapter's features are step-invariant and computed eagerly")
        a.dtype = self.dt
        L.check(self.lib.imh_adapter_op(C.byref(a), self.stream()), descr)

    def pixel_unshuffle(self, image, f, Cp=None, descr="pixel_unshuffle"):
        """image fp32 [N, Cin, H, W] (dense) -> NHWC [N, H / f, W / f, Cp] in the compute dtype: channel c f^2 + dy f + dx of pixel (y, x) is
        image[n, c, y f + dy, x f + dx] (torch's F.pixel_unshuffle, channels last); Cp (default: Cin f^2 rounded up to 8) pads with zeros."""
        self._chk(image, descr + ".image", torch.float32)
        if image.dim() != 4 or not image.is_contiguous():
            raise L.ImhError(f"{descr}: image {tuple(image.shape)} must be dense [N, Cin, H, W]")
        N, Cin, H, W = (int(v) for v in image.shape)
        f = int(f)
        if f < 1 or H % f or W % f:
            raise L.ImhError(f"{descr}: f={f} must divide both sides of {H} x {W}")
        Cp = (Cin * f * f + 7) // 8 * 8 if Cp is None else int(Cp)
        if Cp % 8 or Cp < Cin * f * f:
            raise L.ImhError(f"{descr}: Cp={Cp} must be a multiple of 8 and at least Cin f^2 = {Cin * f * f}")
        out = self.new(N, H // f, W // f, Cp)
        a = L.AdapterArgs()
        a.x, a.y, a.mode, a.N, a.C, a.H, a.W, a.f, a.Cp = image.data_ptr(), out.data_ptr(), L.ADAPTER_UNSHUFFLE, N, Cin, H, W, f, Cp
        self._adapter_op(a, descr)
        return out

    def relu(self, x, out=None, descr="relu"):
        """max(x, 0) over a dense tensor of the compute dtype; out=x runs in place"""
        self._chk(x, descr + ".x"); self._chk(out, descr + ".out")
        if not x.is_contiguous() or x.numel() == 0 or (out is not None and (not out.is_contiguous() or out.shape != x.shape)):
            raise L.ImhError(f"{descr}: x {tuple(x.shape)} (and out) must be dense and of one shape")
        if out is None:
            out = self.new(*x.shape)
        a = L.AdapterArgs()
        a.x, a.y, a.n, a.mode = x.data_ptr(), out.data_ptr(), x.numel(), L.ADAPTER_RELU
        self._adapter_op(a, descr)
        return out

    def avgpool2(self, x, descr="avgpool2"):
        """AvgPool2d(2, 2, ceil_mode=True) over NHWC [N, H, W, C] (dense, C % 8 == 0) -> [N, ceil(H / 2), ceil(W / 2), C]: an edge window
        averages its in-bounds pixels only"""
        self._chk(x, descr + ".x")
        if x.dim() != 4 or not x.is_contiguous() or x.shape[-1] % 8 or x.numel() == 0:
            raise L.ImhError(f"{descr}: x {tuple(x.shape)} must be dense NHWC with C a multiple of 8")
        N, H, W, Cc = (int(v) for v in x.shape)
        out = self.new(N, (H + 1) // 2, (W + 1) // 2, Cc)
        a = L.AdapterArgs()
        a.x, a.y, a.mode, a.N, a.C, a.H, a.W = x.data_ptr(), out.data_ptr(), L.ADAPTER_AVGPOOL2, N, Cc, H, W
        self._adapter_op(a, descr)
        return out

    # ------------------------------------------------------------------ AutoencoderTiny's conv (imh_tinyvae_conv: eager, one launch per conv)
    def tinyvae_conv(self, x, w, bias=None, residual=None, relu=False, up2=False, head=False, tail=False, descr="tinyvae_conv"):
        """one 3 x 3 conv of the tiny VAE decoder (include/imh_tinyvae.h).  Body: x NHWC [B, H, W, 64], w packed [64, 576] -> NHWC
        [B, Ho, Wo, 64] = act(conv(up(x)) + bias + residual); head: x fp32 NCHW [B, 4, H, W], w [64, 36] -> NHWC (tanh clamp, conv, bias,
        ReLU); tail: w [3, 576] -> fp32 NCHW [B, 3, H, W] = 2 (conv + bias) - 1.  The library validates; a refusal raises ImhError."""
        if self.record:
            raise L.ImhError(f"{descr}: imh_tinyvae_conv is no plan kind: the tiny decoder runs eagerly")
        self._chk(x, descr + ".x", torch.float32 if head else None)
        self._chk(w, descr + ".w"); self._chk(bias, descr + ".bias"); self._chk(residual, descr + ".residual")
        cin, cout = (4 if head else 64), (3 if tail else 64)
        ok = x.dim() == 4 and x.is_contiguous() and x.numel() > 0 and (x.shape[1] if head else x.shape[3]) == cin
        if not ok or tuple(w.shape) != (cout, 9 * cin) or not w.is_contiguous():
            raise L.ImhError(f"{descr}: x {tuple(x.shape)} / w {tuple(w.shape)}: expected dense "
                             f"{'NCHW [B, 4, H, W]' if head else 'NHWC [B, H, W, 64]'} and a packed [{cout}, {9 * cin}] weight")
        if bias is not None and (tuple(bias.shape) != (cout,) or not bias.is_contiguous()):
            raise L.ImhError(f"{descr}: bias {tuple(bias.shape)}: expected [{cout}]")
        B, H, W = (int(x.shape[0]), int(x.shape[2]), int(x.shape[3])) if head else (int(v) for v in x.shape[:3])
        Ho, Wo = (2 * H, 2 * W) if up2 else (H, W)
        if residual is not None and (tuple(residual.shape) != (B, Ho, Wo, 64) or not residual.is_contiguous()):
            raise L.ImhError(f"{descr}: residual {tuple(residual.shape)}: expected dense [{B}, {Ho}, {Wo}, 64]")
        out = self.new(B, 3, Ho, Wo, dtype=torch.float32) if tail else self.new(B, Ho, Wo, 64)
        a = L.TinyVaeArgs()
        a.x, a.w, a.bias, a.residual, a.y = x.data_ptr(), w.data_ptr(), self._p(bias), self._p(residual), out.data_ptr()
        a.B, a.H, a.W, a.dtype = B, H, W, self.dt
        a.flags = (L.TINYVAE_RELU if relu else 0) | (L.TINYVAE_UP2 if up2 else 0) | (L.TINYVAE_HEAD if head else 0) | (L.TINYVAE_TAIL if tail else 0)
        L.check(self.lib.imh_tinyvae_conv(C.byref(a), self.stream()), descr)
        return out

    def gather_rows(self, table, idx, add=None, out=None, descr="gather_rows"):
        """out[r] = table[idx[r]] (+ add[r % P]) (IMH_EW_GATHER_ROWS): table [rows, C] and add [P, C] row-major in the compute dtype, idx
        int32 [n] on the device.  The caller has validated the indices on the host (the CLIP text towers' ids and EOS rows are host-known)."""
        self._chk(table, descr + ".table"); self._chk(add, descr + ".add"); self._chk(idx, descr + ".idx", torch.int32)
        n, Cc = idx.numel(), table.shape[1]
        if table.dim() != 2 or table.stride(1) != 1 or idx.dim() != 1 or not idx.is_contiguous() or Cc % 8:
            raise L.ImhError(f"{descr}: table {tuple(table.shape)} must be row-major with a multiple of 8 columns, idx a dense int32 vector")
        if add is not None and (add.dim() != 2 or add.stride(1) != 1 or add.shape[1] != Cc):
            raise L.ImhError(f"{descr}: add {tuple(add.shape)} must be row-major [P, {Cc}]")
        if out is None:
            out = self.new(n, Cc)
        self._chk(out, descr + ".out")
        if out.dim() != 2 or out.stride(1) != 1 or tuple(out.shape) != (n, Cc):
            raise L.ImhError(f"{descr}: out {tuple(out.shape)} must be row-major [{n}, {Cc}]")
        return self.ew(L.EW_GATHER_ROWS, out, a=table, b=idx, w=add, n=n,
                       i=(Cc, table.stride(0), out.stride(0), add.shape[0] if add is not None else 0,
                          add.stride(0) if add is not None else 0, table.shape[0]),
                       descr=descr, nbytes=float(table.element_size()) * n * Cc * (3 if add is not None else 2))

    def silu(self, x, descr="silu"):
        out = self.new(*x.shape)
        return self.ew(L.EW_SILU, out, a=x, n=x.numel(), descr=descr, nbytes=2.0 * x.numel() * x.element_size())

    def concat(self, a, b, descr="concat", freeu=None):
        """NHWC channel concat: a [..., C1], b [..., C2] -> [..., C1 + C2].
        freeu = (scaled, b, s): the FreeU form of the launch (imh.h IMH_EW_CONCAT with i2 > 0; freeu.py states it) on a [B, H, W, C1],
        b [B, H, W, C2] -- the first `scaled` channels of a times b, b through fourier_filter(threshold 1, scale s), then the concat.
        None: the launch as it always was."""
        c1, c2 = a.shape[-1], b.shape[-1]
        pix = a.numel() // c1
        hw = (0, 0, 0)
        if freeu is not None:
            scaled, fb, fs = freeu
            if a.dim() != 4 or b.dim() != 4 or tuple(a.shape[:3]) != tuple(b.shape[:3]) or not (a.is_contiguous() and b.is_contiguous()):
                raise L.ImhError(f"{descr}: the FreeU concat takes dense NHWC [B, H, W, C] pairs of one grid, got {tuple(a.shape)} and {tuple(b.shape)}")
            self._chk(a, f"{descr}.a"); self._chk(b, f"{descr}.b")
            if not 0 <= int(scaled) <= c1 or a.shape[1] < 2 or a.shape[2] < 2 or c1 % 8 or c2 % 8:
                raise L.ImhError(f"{descr}: FreeU over {tuple(a.shape)} | {tuple(b.shape)} with {scaled} scaled channels "
                                 f"(H, W >= 2; channels multiples of 8; 0 <= scaled <= {c1})")
            hw = (int(a.shape[1]), int(a.shape[2]), int(scaled))
        out = self.new(*a.shape[:-1], c1 + c2)
        return self.ew(L.EW_CONCAT, out, a=a, b=b, n=pix, i=(c1, c2) + hw + (0,), descr=descr,
                       f=(float(freeu[1]), float(freeu[2]), 0.0, 0.0) if freeu is not None else (0.0, 0.0, 0.0, 0.0),
                       nbytes=2.0 * out.numel() * out.element_size())

    # ------------------------------------------------------------------ weight prefetch
    def _cold(self, tensors):
        """operands that are parameters (not pool-owned activations) and big enough to matter: every layer's
        weights are read once per forward, i.e. always from HBM unless a previous kernel prefetches them"""
        out = []
        for t in tensors[:2]:
            if t is None or t.numel() * t.element_size() < (256 << 10):
                continue
            if t.untyped_storage().data_ptr() in self._bases:
                continue
            out.append((t.data_ptr(), min(t.numel() * t.element_size(), 0xFFFFFFF0)))
        return out

    PF_CHUNK, PF_CAP_ONLY, PF_BACK = 0, False, 3
    # Round 6: a weight matrix larger than PF_BIG is NOT handed to the launch before it (only its first PF_BIG_CAP bytes, 0 = none).  The one
    # such matrix of the UNet is ff.net.0's [10240, 1280] (26 MB): prefetching it at the tail of the cross-attention's to_out cost that launch
    # 3.8 us (19.4 vs 15.7 us -- the "4 us slower behind the fused cross-attention than behind the self-attention" of round 5's trace) and
    # bought ff.net.0 nothing: its K loops hide their own weight stream (62.2 vs 62.1 us).  -0.28 ms per forward, 559.5 / 561.7 -> 551.6 /
    # 551.3 ms per 30-step denoise in alternating processes (profiles/r06_forward_ab_prefetch_big.json, r06_bench_ab_prefetch_big.txt).
    # Conv weights of that size keep their prefetch: the LDS-halo kernels' two-slot weight rings do not hide a cold stream (8192 x 640 x 17280:
    # 202.9 -> 233.8 us without).  IMH_PF_BIG=0 restores the round-5 behaviour (A/B).
    PF_BIG, PF_BIG_CAP = int(os.environ.get("IMH_PF_BIG", str(14 << 20))), int(os.environ.get("IMH_PF_BIG_CAP", "0"))

    def finalize_prefetch(self):
        """Give every recorded launch the weights of the launch that follows it (tail_prefetch in the kernels):
        a cold weight matrix goes to the nearest earlier op (up to 3 back) whose prefetch slot is still free."""
        if self._pf_done or not self.record:
            return
        self._pf_done = True
        can = (L.OP_GEMM, L.OP_ATTN, L.OP_LAYERNORM, L.OP_GROUPNORM, L.OP_GEMM_DUAL, L.OP_XATTN, L.OP_XATTN_REGIONS)

        def carries(i):
            kind, a = self._ops[i][0], self._ops[i][1]
            if kind not in can:
                return False
            # of the GroupNorm launches only the apply pass touches its prefetch slot (gn_apply_kernel); a table / statistics launch
            # would swallow the pointer and the cold conv weights behind it would never be prefetched
            if kind == L.OP_GROUPNORM and a.mode not in (L.GN_ALL, L.GN_APPLY, L.GN_TABLE_APPLY):
                return False
            return True

        taken = set()
        # PF_CHUNK (bytes; A/B, tools/forward_ab.py `pf_chunk`): a weight matrix larger than this is handed out in pieces -- the first to the
        # nearest earlier launch with a free slot, the next to the one before it, ... (up to PF_BACK launches back); PF_CAP: pieces beyond
        # the first are dropped instead (what is not prefetched is read cold)
        chunk, cap_only, back = self.PF_CHUNK, self.PF_CAP_ONLY, self.PF_BACK
        for j, (kind, args, cold) in enumerate(self._ops):
            for (ptr, nb) in cold:
                pieces = [(ptr, nb)]
                is_conv = kind == L.OP_GEMM and bool(getattr(args, "conv", 0))
                if self.PF_BIG and nb > self.PF_BIG and not is_conv:      # a Linear weight this large: only its first PF_BIG_CAP bytes (0 = none) are prefetched
                    pieces = [(ptr, self.PF_BIG_CAP)] if self.PF_BIG_CAP > 0 else []
                elif chunk and nb > chunk:
                    pieces = [(ptr + o, min(chunk, nb - o)) for o in range(0, nb, chunk)]
                    if cap_only:
                        pieces = pieces[:1]
                # nearest earlier launch with a free slot (measured better than handing big matrices to a longer,
                # earlier kernel: 27.0 vs 27.3 ms per forward)
                i = j - 1
                for (pp, pn) in pieces:
                    while i > max(j - 1 - back, -1) and (i in taken or not carries(i)):
                        i -= 1
                    if i <= max(j - 1 - back, -1):
                        break
                    a = self._ops[i][1]
                    tgt = a[0] if self._ops[i][0] == L.OP_GEMM_DUAL else a
                    tgt.pf_ptr, tgt.pf_bytes = pp, pn
                    ref = C.cast(a, C.c_void_p) if self._ops[i][0] == L.OP_GEMM_DUAL else C.byref(a)
                    L.check(self.lib.imh_plan_update(self.plan, i, ref), "imh_plan_update")
                    taken.add(i)
                    i -= 1
        return len(taken)

    # ------------------------------------------------------------------ plans
    def run(self):
        self.finalize_prefetch()
        L.check(self.lib.imh_plan_run(self.plan, self.stream()), "imh_plan_run")

    def capture(self):
        """Capture the recorded plan into a hipGraph (needs a non-default stream)."""
        self.finalize_prefetch()
        s = torch.cuda.Stream(self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            L.check(self.lib.imh_plan_capture(self.plan, C.c_void_p(s.cuda_stream)), "imh_plan_capture")
        torch.cuda.current_stream(self.device).wait_stream(s)
        self.captured = True

    def replay(self):
        if self.captured:
            L.check(self.lib.imh_plan_replay(self.plan, self.stream()), "imh_plan_replay")
        else:
            self.run()

    def time_ops(self):
        self.finalize_prefetch()
        n = self.lib.imh_plan_size(self.plan)
        ms = (C.c_float * n)()
        L.check(self.lib.imh_plan_time_ops(self.plan, self.stream(), ms, n), "imh_plan_time_ops")
        return list(ms)

    def __del__(self):
        try:
            if self.plan:
                self.lib.imh_plan_destroy(self.plan)
                self.plan = None
        except Exception:
            pass
