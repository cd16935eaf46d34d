"""CPU: the reference's OWN denoise loop (ip_adapter/custom_pipelines.py __call__, executed verbatim through
oracle/refshim.py on a restated base class; its final latents stored in tests/golden/refpin_denoise_loop.pt by
oracle/gen_refpins.py) against the oracle's restatement of it (oracle/pipeline.py).  Pins row a11 of SURVEY.md section
8 -- scale gating window, CFG order [uncond | cond], guidance rescale, micro-conditioning time_ids, scheduler call order
-- to the reference code itself.  The UNet and the scheduler are the oracle's (diffusers is absent); the reference run
carried the REFERENCE's processor classes with the same seeded weights."""
import os

import pytest
import torch

from oracle.detfill import det_fill
from oracle.gen_refpins import LOOP_CASES, loop_inputs
from oracle.pipeline import denoise as oracle_denoise
from oracle.schedulers import DDIMScheduler, EulerDiscreteScheduler
from oracle.sdxl_unet import UNet2DConditionModel, tiny_config
from conftest import GOLDEN


@pytest.mark.parametrize("kind,kw", LOOP_CASES)
def test_reference_loop_equals_oracle_loop(kind, kw):
    g = torch.load(os.path.join(GOLDEN, "refpin_denoise_loop.pt"))
    assert g["cases"] == LOOP_CASES
    ref = g["latents"][LOOP_CASES.index((kind, kw))]
    cfg = tiny_config()
    lat, pe, ne, po, no = loop_inputs(cfg)
    with torch.no_grad():
        # the oracle loop with the ORACLE processor classes carrying the weights the reference run had
        from oracle import modules as om
        from oracle.pipeline import install_ip_processors
        u2 = det_fill(UNet2DConditionModel(cfg), 5).eval()
        for n, p in install_ip_processors(u2, num_tokens=4, scale=0.8).items():
            if isinstance(p, om.IPAttnProcessor2_0):
                det_fill(p, 7, prefix=n)
        mine = oracle_denoise(u2, DDIMScheduler() if kind == "ddim" else EulerDiscreteScheduler(), lat.clone(), pe, ne, po, no,
                              256, 256, num_inference_steps=4, guidance_scale=5.0, **kw)
    assert ref.shape == mine.shape
    err = ((ref - mine).pow(2).mean().sqrt() / mine.pow(2).mean().sqrt()).item()
    assert err < 1e-5, err
