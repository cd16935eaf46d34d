"""Time the HIP VAE per 1024^2 image, fp16 module (fp32 mode, as the reference upcasts) and bf16 (native), tiled and untiled.
python tools/vae_time.py [decode|encode]   (default decode)"""
import sys, time, torch
sys.path.insert(0, '.')
from imagharmony_amd.vae import AutoencoderKL, decode_latents
DEV='cuda:0'
mode = sys.argv[1] if len(sys.argv) > 1 else "decode"
if mode not in ("decode", "encode"):
    raise SystemExit("usage: python tools/vae_time.py [decode|encode]")
lat = torch.randn(1, 4, 128, 128, generator=torch.Generator().manual_seed(0)).to(DEV) * 0.13025
img = (torch.rand(1, 3, 1024, 1024, generator=torch.Generator().manual_seed(0)) * 2 - 1).to(DEV)
for mdt in (torch.float16, torch.bfloat16):
    vae = AutoencoderKL(with_encoder=mode == "encode").init_random_(1).to(DEV, mdt)
    run = (lambda: vae.encode_moments(img)) if mode == "encode" else (lambda: decode_latents(vae, lat))
    for tiled in (False, True):
        vae.enable_tiling(tiled)
        run(); torch.cuda.synchronize()
        t=time.perf_counter()
        for _ in range(3): run()
        torch.cuda.synchronize()
        print(mode, mdt, vae.precision_for(), 'tiled' if tiled else 'untiled', (time.perf_counter()-t)/3*1e3, 'ms')
