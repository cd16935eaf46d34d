"""LoRA for the SDXL UNet, merged into the weights by one grouped launch (include/imh_lora.h, csrc/lora.hip).

A denoise step is one replayed hipGraph; an unmerged LoRA would add two launches per adapted Linear, more than a thousand per step.  So a
LoRA is MERGED: the step graph stays launch for launch what it is, and what costs is the merge -- every ``set_adapters`` / ``load`` /
``delete`` / ``enable`` / ``disable`` is ONE ``apply()``, which is one host-to-device copy of the strengths and one kernel launch over
every touched weight:

    W[n, k] = round_T( fp32(W0[n, k]) + sum_j U[n, j] * (g[j] * D[j, k]) )

W0 is a snapshot of the weight taken the first time an adapter touches it (repeated fuse / unfuse in bf16 would drift: the merge always
starts from the snapshot and rounds once), U / D the ``up`` / ``down`` factors of every adapter on that module concatenated along the
rank, in fp32, and g[j] = adapter_weight * alpha / rank of the adapter that owns column j (0 when it is inactive).

The kernel stores into the weights behind torch's back, so apply() bumps ``_version`` of every touched parameter -- every packed,
folded, interleaved or stacked copy of a weight is keyed by derived.vkey = (data_ptr, _version) and rebuilds itself (derived.py) -- and
increments ``unet.lora_epoch``, which DenoiseEngine compares with the value it saw at set_conditioning (its K / V caches, aug_emb,
time-embedding rows and recorded plans derive from the weights).

Key names.  Three published layouts are read: diffusers / PEFT (``[unet.]<module>.lora_A.weight`` / ``lora_B.weight`` and
``.lora.down.weight`` / ``.lora.up.weight``), kohya with diffusers module paths (``lora_unet_<module with _>.lora_down.weight``) and kohya
with the original SDXL (SGM) module paths, which is what published SDXL LoRAs carry.  The tables are generated from the model's own
modules (name_tables) and kohya keys are looked up in them, never parsed at the underscores.  diffusers is not a dependency: the
tables restate the published layouts and tests/test_lora_host.py checks them structurally against tests/golden/sdxl_unet_manifest.txt.

Not built (refused where reachable): text-encoder LoRA, LoRA on a ControlNetModel or T2IAdapter, per-block adapter weights, a per-call
``scale`` (cross_attention_kwargs), DoRA / LoHa / LoKr / Tucker, bias deltas."""
import ctypes as C
import re

import numpy as np
import torch

from . import lib as L

_DOWN = (".lora_A.weight", ".lora.down.weight", ".lora_down.weight")
_UP = (".lora_B.weight", ".lora.up.weight", ".lora_up.weight")
_REFUSED = (("dora_scale", "DoRA"), ("hada_", "LoHa"), ("lokr_", "LoKr"), ("lora_mid", "Tucker (lora_mid)"))
_BIAS = (".bias", ".diff_b", ".lora_B.bias")


# ------------------------------------------------------------------------------------------------------------------ name tables
def adaptable_modules(unet):
    """{module name: module} of the Linear / Conv2d weight holders of a UNet (unet.py's own classes: the attention processors' extra
    projections are not part of the UNet proper), in module order"""
    from .unet import Conv2d, Linear
    return {n: m for n, m in unet.named_modules() if isinstance(m, (Linear, Conv2d)) and ".processor" not in n}


def _meta_unet(cfg):
    from .unet import UNet2DConditionModel
    with torch.device("meta"):
        return UNet2DConditionModel(cfg)


def sgm_names(unet):
    """{diffusers module name: the original SDXL (SGM) name} for every adaptable module, from the model's own block structure:
    input_blocks count conv_in, then every down-block layer and downsampler; output_blocks every up-block layer, the upsampler riding as
    the last member of its layer's block"""
    pre = {"conv_in": "input_blocks.0.0", "time_embedding.linear_1": "time_embed.0", "time_embedding.linear_2": "time_embed.2",
           "add_embedding.linear_1": "label_emb.0.0", "add_embedding.linear_2": "label_emb.0.2", "conv_out": "out.2"}
    idx = 1
    for bi, blk in enumerate(unet.down_blocks):
        for j in range(len(blk.resnets)):
            pre[f"down_blocks.{bi}.resnets.{j}"] = f"input_blocks.{idx}.0"
            if blk.has_attn:
                pre[f"down_blocks.{bi}.attentions.{j}"] = f"input_blocks.{idx}.1"
            idx += 1
        if blk.downsamplers is not None:
            pre[f"down_blocks.{bi}.downsamplers.0.conv"] = f"input_blocks.{idx}.0.op"
            idx += 1
    pre["mid_block.resnets.0"], pre["mid_block.attentions.0"], pre["mid_block.resnets.1"] = "middle_block.0", "middle_block.1", "middle_block.2"
    idx = 0
    for bi, blk in enumerate(unet.up_blocks):
        for j in range(len(blk.resnets)):
            pre[f"up_blocks.{bi}.resnets.{j}"] = f"output_blocks.{idx}.0"
            if blk.has_attn:
                pre[f"up_blocks.{bi}.attentions.{j}"] = f"output_blocks.{idx}.1"
            if blk.upsamplers is not None and j == len(blk.resnets) - 1:
                pre[f"up_blocks.{bi}.upsamplers.0.conv"] = f"output_blocks.{idx}.{1 + int(blk.has_attn)}.conv"
            idx += 1
    res = {"conv1": "in_layers.2", "time_emb_proj": "emb_layers.1", "conv2": "out_layers.3", "conv_shortcut": "skip_connection"}
    out = {}
    for name in adaptable_modules(unet):
        if name in pre:
            out[name] = pre[name]
            continue
        head = max((p for p in pre if name.startswith(p + ".")), key=len, default=None)
        if head is None:
            raise KeyError(f"{name}: no place in the SGM layout")
        tail = name[len(head) + 1:]
        out[name] = pre[head] + "." + (res[tail] if ".resnets." in head else tail)      # a transformer's inner names are the same on both sides
    return out


def name_tables(unet_or_cfg):
    """-> (diffusers table, SGM table): {kohya key stem ``lora_unet_<path with _>``: diffusers module name}.  unet_or_cfg: a UNet, or a
    UNetConfig (the model is then built on the meta device: no memory)"""
    unet = unet_or_cfg if hasattr(unet_or_cfg, "down_blocks") else _meta_unet(unet_or_cfg)
    stem = lambda s: "lora_unet_" + s.replace(".", "_")
    return {stem(n): n for n in adaptable_modules(unet)}, {stem(s): n for n, s in sgm_names(unet).items()}


# ------------------------------------------------------------------------------------------------------------------ parsing
def _split(key):
    """-> (module part, "down" | "up" | "alpha") or None for a key that is no LoRA factor"""
    for sufs, what in ((_DOWN, "down"), (_UP, "up"), ((".alpha",), "alpha")):
        for s in sufs:
            if key.endswith(s):
                return key[:-len(s)], what
    return None


def parse_state_dict(sd, unet_or_cfg, text_encoder="error"):
    """A LoRA state dict in any of the namings above -> ({unet module name: (down fp32, up fp32, alpha or None)}, skipped keys).
    The factors keep their shapes (a conv pair stays 4-D); LoRAState checks them against the module.
    NotImplementedError (naming the key): DoRA, LoHa, LoKr, Tucker, bias deltas, text-encoder keys unless text_encoder="skip".
    KeyError (listing the keys): keys that match no module, a factor without its partner."""
    if text_encoder not in ("error", "skip"):
        raise ValueError(f'text_encoder must be "error" or "skip", not {text_encoder!r}')
    unet = unet_or_cfg if hasattr(unet_or_cfg, "down_blocks") else _meta_unet(unet_or_cfg)
    mods = adaptable_modules(unet)
    t_dif, t_sgm = name_tables(unet)
    found, skipped, unknown = {}, [], []
    for key in sd:
        for frag, what in _REFUSED:
            if frag in key:
                raise NotImplementedError(f"{key}: {what} is not built (plain LoRA / LoCon pairs only)")
        if key.startswith(("lora_te", "text_encoder")):
            if text_encoder != "skip":
                raise NotImplementedError(f'{key}: text-encoder LoRA is not built (text_encoder="skip" leaves these keys out)')
            skipped.append(key)
            continue
        if key.endswith(_BIAS):
            raise NotImplementedError(f"{key}: bias deltas are not built")
        sp = _split(key)
        if sp is None:
            unknown.append(key)
            continue
        part, what = sp
        if part.startswith("lora_unet_"):
            name = t_dif.get(part) or t_sgm.get(part)
        else:
            name = part[5:] if part.startswith("unet.") else part
            name = name if name in mods else None
        if name is None:
            unknown.append(key)
            continue
        found.setdefault(name, {})[what] = sd[key]
    if unknown:
        raise KeyError(f"{len(unknown)} key(s) match no module of this UNet: {sorted(unknown)}")
    half = sorted(n for n, f in found.items() if "down" not in f or "up" not in f)
    if half:
        raise KeyError(f"module(s) with one factor of the pair or an alpha alone: {half}")
    canon = {}
    for name in mods:                                    # module order
        if name in found:
            f = found[name]
            alpha = f.get("alpha")
            canon[name] = (f["down"].detach().to("cpu", torch.float32), f["up"].detach().to("cpu", torch.float32),
                           None if alpha is None else float(alpha))
    return canon, skipped


def _factors_2d(name, w_shape, down, up):
    """the pair as D [r, K], U [N, r] in the master layout's own order, or None when the shapes do not fit the module's weight"""
    N, K = int(w_shape[0]), int(np.prod(w_shape[1:]))
    r = int(down.shape[0]) if down.dim() >= 2 else -1
    ok = r >= 1 and down.dim() in (2, len(w_shape)) and up.dim() >= 2 and down.numel() == r * K and tuple(up.shape[:2]) == (N, r) and up.numel() == N * r
    if ok and down.dim() == 4 and len(w_shape) == 4:
        ok = tuple(down.shape[1:]) == tuple(w_shape[1:])
    return (down.reshape(r, K).contiguous(), up.reshape(N, r).contiguous()) if ok else None


# ------------------------------------------------------------------------------------------------------------------ state
class LoRAState:
    """What ``unet._lora`` holds: the adapters by name, a snapshot of every touched weight, the concatenated fp32 factors per module, the
    device item table with its tile prefix, and one device ``g`` array.  ``layout`` is the bookkeeping the item table is built from:
    [(module name, [(adapter name, rank, alpha / rank, offset into g)])] in module order, the adapters of a module in load order; it is
    rebuilt on load and delete, not on a weight change."""

    def __init__(self, unet):
        self.unet = unet
        self.adapters = {}           # name -> dict(modules={module: (D [r, K], U [N, r], scale)}, weight, active, rank)
        self.snap = {}               # module name -> T snapshot (a clone of the weight)
        self.enabled = True
        self.layout = []
        self.g_host = np.zeros(0, np.float32)
        self.U, self.D = {}, {}
        self.items = self.items_dev = self.prefix_dev = self.g_dev = None
        self.total_tiles = 0
        self.dtype = None

    # -- what a test without a device replaces --
    def _check_weights(self, names):
        """ValueError unless every touched weight is a contiguous bf16 / fp16 tensor on one GPU, all of one dtype"""
        mods = adaptable_modules(self.unet)
        ws = [mods[n].weight for n in names]
        bad = [n for n, w in zip(names, ws) if w.device.type != "cuda" or w.dtype not in (torch.bfloat16, torch.float16) or not w.is_contiguous()]
        if bad:
            raise ValueError(f"LoRA merges on the GPU into bf16 / fp16 weights: {len(bad)} touched parameter(s) are not (e.g. {bad[:3]}); "
                             f"move the UNet first (unet.to(device, dtype))")
        held = [self.dtype] if self.dtype is not None else []
        if len({w.dtype for w in ws} | set(held)) > 1 or len({w.device for w in ws}) > 1:
            raise ValueError("the touched weights must share one dtype and one device")

    def _weights(self):
        mods = adaptable_modules(self.unet)
        return {n: mods[n].weight for n in self.snap}

    # -- adapters --
    def add(self, name, canon):
        """a parsed adapter becomes active at weight 1.0; one apply()"""
        if name in self.adapters:
            raise ValueError(f"adapter {name!r} is already loaded: delete_adapters first, or pick another adapter_name")
        mods = adaptable_modules(self.unet)
        entry, misfit = {}, []
        for mod, (down, up, alpha) in canon.items():
            f = _factors_2d(mod, tuple(mods[mod].weight.shape), down, up)
            if f is None:
                misfit.append(f"{mod}: down {tuple(down.shape)}, up {tuple(up.shape)} for a weight {tuple(mods[mod].weight.shape)}")
                continue
            r = f[0].shape[0]
            entry[mod] = (f[0], f[1], 1.0 if alpha is None else float(alpha) / r)
        if misfit:
            raise KeyError(f"factor shapes do not fit the module: {misfit}")
        if not entry:
            raise KeyError("the state dict holds no UNet LoRA factors")
        self._check_weights(list(entry))                 # before anything changes
        with torch.no_grad():
            for mod in entry:
                if mod not in self.snap:
                    self.snap[mod] = mods[mod].weight.detach().clone()
        self.dtype = next(iter(self.snap.values())).dtype
        ranks = sorted({int(f[0].shape[0]) for f in entry.values()})
        self.adapters[name] = dict(modules=entry, weight=1.0, active=True, rank=ranks[0] if len(ranks) == 1 else ranks)
        self._rebuild()
        self.apply()

    def delete(self, names):
        names = [names] if isinstance(names, str) else list(names)
        missing = [n for n in names if n not in self.adapters]
        if missing:
            raise ValueError(f"no adapter(s) {missing}; loaded: {list(self.adapters)}")
        for n in names:
            del self.adapters[n]
        self._rebuild()
        self.apply()

    def set_adapters(self, names, weights=None):
        names = [names] if isinstance(names, str) else list(names)
        if weights is None:
            weights = [1.0] * len(names)
        elif not isinstance(weights, (list, tuple)):
            weights = [weights] * len(names)
        if len(weights) != len(names):
            raise ValueError(f"{len(weights)} adapter_weights for {len(names)} adapters")
        for w in weights:
            if isinstance(w, dict):
                raise NotImplementedError("per-block adapter weights (a dict per adapter) are not built: one number per adapter")
        missing = [n for n in names if n not in self.adapters]
        if missing:
            raise ValueError(f"no adapter(s) {missing}; loaded: {list(self.adapters)}")
        for n, a in self.adapters.items():
            a["active"] = n in names
        for n, w in zip(names, weights):
            self.adapters[n]["weight"] = 1.0 if w is None else float(w)
        self.apply()

    def set_enabled(self, on):
        self.enabled = bool(on)
        self.apply()

    def active(self):
        return [n for n, a in self.adapters.items() if a["active"]] if self.enabled else []

    # -- bookkeeping --
    def _rebuild(self):
        """layout and g_host from the adapters; every module that has a snapshot keeps an item (with no adapter left on it: rank 0, the
        merge copies the snapshot back)"""
        order = [n for n in adaptable_modules(self.unet) if n in self.snap]
        self.layout, off = [], 0
        for mod in order:
            cols = []
            for an, a in self.adapters.items():
                if mod in a["modules"]:
                    D, _, scale = a["modules"][mod]
                    cols.append((an, int(D.shape[0]), scale, off))
                    off += int(D.shape[0])
            self.layout.append((mod, cols))
        self.g_host = np.zeros(off, np.float32)
        self._upload()

    def _fill_g(self):
        for _, cols in self.layout:
            for an, r, scale, off in cols:
                a = self.adapters[an]
                self.g_host[off:off + r] = np.float32(a["weight"] * scale) if (self.enabled and a["active"]) else np.float32(0.0)
        return self.g_host

    def factors(self, mod):
        """(U [N, R], D [R, K]) of a module on the CPU in fp32, concatenated as the layout says, or (None, None) at rank 0"""
        cols = dict(self.layout)[mod]
        if not cols:
            return None, None
        return (torch.cat([self.adapters[an]["modules"][mod][1] for an, _, _, _ in cols], 1).contiguous(),
                torch.cat([self.adapters[an]["modules"][mod][0] for an, _, _, _ in cols], 0).contiguous())

    def _upload(self):
        """the device side of the layout: concatenated factors, the item table, the tile prefix and the g array"""
        lib = L.load()
        ws = self._weights()
        dev = next(iter(ws.values())).device
        self.U, self.D = {}, {}
        n = len(self.layout)
        self.g_dev = torch.zeros(max(len(self.g_host), 1), dtype=torch.float32, device=dev)
        self.items = (L.LoraItem * n)()
        prefix = [0]
        for i, (mod, cols) in enumerate(self.layout):
            w, it = ws[mod], self.items[i]
            N, K = int(w.shape[0]), int(w[0].numel())
            R = sum(r for _, r, _, _ in cols)
            it.base, it.dst, it.N, it.K, it.R, it.ld_base, it.ld_dst = self.snap[mod].data_ptr(), w.data_ptr(), N, K, R, K, K
            it.ldu, it.ldd = R, K
            if R:
                U, D = self.factors(mod)
                self.U[mod], self.D[mod] = U.to(dev), D.to(dev)
                it.U, it.D, it.g = self.U[mod].data_ptr(), self.D[mod].data_ptr(), self.g_dev.data_ptr() + 4 * cols[0][3]
            prefix.append(prefix[-1] + lib.imh_lora_merge_tiles(N, K))
        self.total_tiles = prefix[-1]
        self.items_dev = torch.frombuffer(bytearray(bytes(self.items)), dtype=torch.uint8).to(dev) if n else None
        self.prefix_dev = torch.tensor(prefix, dtype=torch.int32, device=dev)

    # -- the merge --
    @torch.no_grad()
    def apply(self):
        """g (one host-to-device copy; inactive adapters get 0), the merge launch, _version of every touched parameter, unet.lora_epoch"""
        g = self._fill_g()
        if self.layout:
            lib = L.load()
            ws = self._weights()
            dev = self.g_dev.device
            if len(g):
                self.g_dev[:len(g)].copy_(torch.from_numpy(g))
            a = L.LoraMergeArgs()
            a.items_host, a.items_dev, a.tile_start_dev = C.addressof(self.items), self.items_dev.data_ptr(), self.prefix_dev.data_ptr()
            a.n_items, a.total_tiles = len(self.layout), self.total_tiles
            a.dtype = L.IMH_DT_BF16 if self.dtype == torch.bfloat16 else L.IMH_DT_F16
            with torch.cuda.device(dev):
                L.check(lib.imh_lora_merge(C.byref(a), torch.cuda.current_stream(dev).cuda_stream), "imh_lora_merge")
            for w in ws.values():
                torch.autograd.graph.increment_version(w)      # a raw HIP store bumps nothing: the derived copies are keyed by it
        self.unet.lora_epoch = getattr(self.unet, "lora_epoch", 0) + 1

    def report(self, name, skipped):
        a = self.adapters[name]
        return dict(adapter_name=name, modules=list(a["modules"]), rank=a["rank"], skipped=list(skipped))


# ------------------------------------------------------------------------------------------------------------------ the public surface
def _read(path_or_state_dict):
    if isinstance(path_or_state_dict, dict):
        return path_or_state_dict
    path = str(path_or_state_dict)
    if not path.endswith(".safetensors"):
        raise ValueError(f"{path}: a .safetensors file or a state dict")
    from safetensors.torch import load_file
    return load_file(path, device="cpu")


class LoRAMixin:
    """diffusers' LoRA methods on UNet2DConditionModel, with their names and meanings; every state change is one LoRAState.apply()"""
    lora_epoch = 0          # counts merges: DenoiseEngine compares it with the value it saw at set_conditioning
    _lora = None

    def _lora_state(self):
        if self._lora is None:
            raise ValueError("no LoRA is loaded: load_lora_weights first")
        return self._lora

    def load_lora_weights(self, path_or_state_dict, adapter_name=None, text_encoder="error"):
        """-> report: dict(adapter_name, modules touched, rank, skipped keys).  The new adapter is active at weight 1.0."""
        canon, skipped = parse_state_dict(_read(path_or_state_dict), self, text_encoder=text_encoder)
        st = self._lora if self._lora is not None else LoRAState(self)
        if adapter_name is None:
            adapter_name = next(f"default_{i}" for i in range(len(st.adapters) + 1) if f"default_{i}" not in st.adapters)
        st.add(adapter_name, canon)
        self._lora = st
        return st.report(adapter_name, skipped)

    def set_adapters(self, names, adapter_weights=None):
        self._lora_state().set_adapters(names, adapter_weights)

    def get_active_adapters(self):
        return self._lora.active() if self._lora is not None else []

    def get_list_adapters(self):
        return list(self._lora.adapters) if self._lora is not None else []

    def delete_adapters(self, names):
        self._lora_state().delete(names)

    def disable_lora(self):
        self._lora_state().set_enabled(False)

    def enable_lora(self):
        self._lora_state().set_enabled(True)

    def unload_lora_weights(self):
        """the snapshots' bits come back exactly (one merge at strength 0) and all LoRA memory is freed"""
        if self._lora is not None:
            self._lora.set_enabled(False)
            self._lora = None

    def fuse_lora(self):
        """keeps the merged weights and frees snapshots, factors and adapters; irreversible"""
        self._lora_state()
        self._lora = None

    def unfuse_lora(self):
        raise NotImplementedError("fuse_lora frees the snapshots: there is nothing to unfuse from (keep the adapters loaded and use "
                                  "disable_lora / unload_lora_weights instead)")


class LoRAPipelineMixin:
    """the same methods on the pipelines: they delegate to the UNet.  Text-encoder LoRA is not built (text_encoder="skip" leaves such keys
    out of a file); a ControlNet or T2I-Adapter on the pipe is not touched."""

    def load_lora_weights(self, path_or_state_dict, adapter_name=None, text_encoder="error"):
        return self.unet.load_lora_weights(path_or_state_dict, adapter_name=adapter_name, text_encoder=text_encoder)

    def set_adapters(self, names, adapter_weights=None):
        self.unet.set_adapters(names, adapter_weights)

    def get_active_adapters(self):
        return self.unet.get_active_adapters()

    def get_list_adapters(self):
        return {"unet": self.unet.get_list_adapters()}

    def delete_adapters(self, names):
        self.unet.delete_adapters(names)

    def disable_lora(self):
        self.unet.disable_lora()

    def enable_lora(self):
        self.unet.enable_lora()

    def unload_lora_weights(self):
        self.unet.unload_lora_weights()

    def fuse_lora(self):
        self.unet.fuse_lora()

    def unfuse_lora(self):
        self.unet.unfuse_lora()


def synthetic_adapter(unet_or_cfg, rank, seed=0, select=None, alpha=None, std=0.02, naming="diffusers"):
    """a seeded random adapter over the modules select(name) keeps (default: all adaptable ones) -- examples/, tools/lora_time.py and the
    tests.  naming: "diffusers" (``unet.<module>.lora_A.weight``), "peft_old" (``.lora.down.weight``), "kohya" or "sgm"."""
    unet = unet_or_cfg if hasattr(unet_or_cfg, "down_blocks") else _meta_unet(unet_or_cfg)
    gen = torch.Generator("cpu").manual_seed(seed)
    sgm = sgm_names(unet) if naming == "sgm" else None
    sd = {}
    for name, m in adaptable_modules(unet).items():
        if select is not None and not select(name):
            continue
        shp = tuple(m.weight.shape)
        down = torch.randn((rank,) + shp[1:], generator=gen) * std
        up = torch.randn((shp[0], rank) + (1,) * (len(shp) - 2), generator=gen) * std
        if naming == "diffusers":
            kd, ku, ka = f"unet.{name}.lora_A.weight", f"unet.{name}.lora_B.weight", f"unet.{name}.alpha"
        elif naming == "peft_old":
            kd, ku, ka = f"{name}.lora.down.weight", f"{name}.lora.up.weight", f"{name}.alpha"
        else:
            stem = "lora_unet_" + (sgm[name] if naming == "sgm" else name).replace(".", "_")
            kd, ku, ka = stem + ".lora_down.weight", stem + ".lora_up.weight", stem + ".alpha"
        sd[kd], sd[ku] = down, up
        if alpha is not None:
            sd[ka] = torch.tensor(float(alpha))
    return sd


ATTN_FF_PROJ = re.compile(r"\.(to_q|to_k|to_v|to_out\.0|ff\.net\.0\.proj|ff\.net\.2|proj_in|proj_out)$")      # the usual targets of an SDXL LoRA
