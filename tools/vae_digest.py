"""sha256 of the HIP VAE's output bytes per case, to compare two versions of the package bit for bit on one library binary.
python tools/vae_digest.py [PACKAGE_DIR]   (the imagharmony_amd/ directory to import; default: this tree's.  IMH_LIB_PATH names the library
when PACKAGE_DIR holds none.)  Tiny configuration, random weights, seeded inputs; prints one JSON object {case: digest}."""
import hashlib, json, os, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "imagharmony_amd"))
sys.path[:0] = [os.path.dirname(pkg), ROOT]
from imagharmony_amd.vae import AutoencoderKL, VAEConfig
from oracle.vae import tiny_vae_config
DEV = 'cuda:0'
ocfg = tiny_vae_config()
cfg = VAEConfig(**{k: getattr(ocfg, k) for k in VAEConfig.__dataclass_fields__})
rand = lambda *s: torch.randn(*s, generator=torch.Generator().manual_seed(sum(s))).to(DEV)
# (module dtype, precision): the shapes reach the untiled path, ragged token counts (324 / 425: no multiple of 64, 16 or 4) and ragged tiles
CASES = {"decode": ([(torch.bfloat16, "native"), (torch.float16, "native"), (torch.float16, None)],
                    [((2, 4, 32, 32), False), ((2, 4, 18, 18), False), ((1, 4, 42, 38), True)]),
         "encode": ([(torch.bfloat16, "native"), (torch.float32, None)],
                    [((2, 3, 256, 256), False), ((1, 3, 200, 136), False), ((1, 3, 448, 328), True)])}
out = {}
for mode, (mods, inputs) in CASES.items():
    for mdt, prec in mods:
        vae = AutoencoderKL(cfg, with_encoder=mode == "encode").init_random_(1).to(DEV, mdt)
        for shape, tiled in inputs:
            vae.enable_tiling(tiled)
            x = rand(*shape)
            y = vae.decode(x, precision=prec) if mode == "decode" else vae.encode_moments(x.tanh(), precision=prec)
            name = f"{mode} {str(mdt)[6:]}->{vae.precision_for(prec)} {'x'.join(map(str, shape))}{' tiled' if tiled else ''}"
            out[name] = hashlib.sha256(y.contiguous().cpu().numpy().tobytes()).hexdigest() + f" {tuple(y.shape)}"
print(json.dumps(out, indent=1))
