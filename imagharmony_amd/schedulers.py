"""Schedulers of the denoise loop, restated for a device-resident loop.

The reference calls ``scheduler.set_timesteps / scale_model_input / step`` on whatever scheduler the SDXL
pipeline ships (ip_adapter/custom_pipelines.py:250-252,334,357): EulerDiscrete for stock SDXL-base (what
test.py runs), DDIM eta=0 per BASELINE.json.  Both are LINEAR updates
``x' = cx*x + ce*eps`` with an optional input scale, so each scheduler reduces to three per-step tables
that the HIP kernels read from device memory (csrc/elementwise.hip EW_CONV_IN / EW_CFG_STEP):

    timesteps[i], in_scale[i] (scale_model_input), (cx[i], ce[i]) (step), init_noise_sigma.

Same public surface as diffusers for the calls the reference makes, so they also work as plain
host-side schedulers (``step`` on tensors) in tests.

DPM-Solver++ 2M (with Karras sigmas, or as the SDE variant) and Euler ancestral need the previous data prediction and per-step noise:
they hand over a six-column table ``coef6`` instead of ``coef`` and step through EW_CFG_MSTEP (second half of this file).
"""
import numpy as np
import torch


def _alphas_cumprod(n_train=1000, beta_start=0.00085, beta_end=0.012):
    betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, n_train, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0).double()


class _Base:
    order = 1
    num_train_timesteps = 1000

    def tables(self):
        """-> dict(timesteps f32[n], in_scale f32[n] | None, coef f32[n, 2], init_noise_sigma float)"""
        raise NotImplementedError

    def scale_model_input(self, x, t):
        i = self._index(t)
        s = self.tables()["in_scale"]
        return x if s is None else x * float(s[i])

    def step(self, eps, t, x, return_dict=False, **kw):
        i = self._index(t)
        c = self.tables()["coef"][i]
        return ((float(c[0]) * x.float() + float(c[1]) * eps.float()).to(x.dtype),)

    def _index(self, t):
        ts = self.timesteps.tolist()
        return ts.index(float(t) if isinstance(ts[0], float) else int(t))

    def add_noise_coefficients(self, t_start):
        """(a, b) of ``scheduler.add_noise(x, noise, timesteps[t_start]) == a * x + b * noise`` (image-to-image: the initial latents
        start at step t_start of the schedule set by set_timesteps)"""
        raise NotImplementedError

    def add_noise(self, x, noise, t_start):
        """host-side add_noise at step index t_start, in fp32 as diffusers computes it"""
        a, b = self.add_noise_coefficients(t_start)
        return x.float() * a + noise.float() * b


def get_timesteps(scheduler, num_inference_steps, strength):
    """diffusers 0.30 StableDiffusionXLImg2ImgPipeline.get_timesteps (denoising_start=None) -> (timesteps[t_start:], t_start), after
    scheduler.set_timesteps(num_inference_steps): init = min(int(n * strength), n), t_start = max(n - init, 0).  A schedule that
    truncates to no step raises ValueError, as diffusers' check does."""
    if not 0.0 <= float(strength) <= 1.0:
        raise ValueError(f"strength must be in [0.0, 1.0], got {strength}")
    n = int(num_inference_steps)
    init = min(int(n * strength), n)
    t_start = max(n - init, 0)
    if n - t_start < 1:
        raise ValueError(f"strength {strength} with num_inference_steps {n} leaves no denoising step (num_inference_steps * strength < 1)")
    return scheduler.timesteps[t_start * scheduler.order:], t_start


class DDIMScheduler(_Base):
    """scaled_linear betas, clip_sample=False, set_alpha_to_one=False, steps_offset=1, leading spacing,
    epsilon prediction, eta=0."""
    init_noise_sigma = 1.0

    def __init__(self):
        self.alphas_cumprod = _alphas_cumprod()
        self.timesteps = None

    def set_timesteps(self, n, device=None):
        self.num_inference_steps = n
        r = self.num_train_timesteps // n
        self.timesteps = torch.from_numpy((np.arange(0, n) * r).round()[::-1].copy().astype(np.int64) + 1)
        self._tab = None

    def tables(self):
        if getattr(self, "_tab", None) is None:
            n = self.num_inference_steps
            r = self.num_train_timesteps // n
            ac = self.alphas_cumprod
            coef = torch.zeros(n, 2, dtype=torch.float64)
            for i, t in enumerate(self.timesteps.tolist()):
                a = ac[t]
                ap = ac[t - r] if t - r >= 0 else ac[0]
                cx = (ap / a).sqrt()
                coef[i, 0] = cx
                coef[i, 1] = (1 - ap).sqrt() - cx * (1 - a).sqrt()
            self._tab = dict(timesteps=self.timesteps.float(), in_scale=None, coef=coef.float(), init_noise_sigma=1.0)
        return self._tab

    def add_noise_coefficients(self, t_start):
        """diffusers DDIMScheduler.add_noise: (sqrt(abar_t), sqrt(1 - abar_t)) at t = timesteps[t_start], in fp32"""
        ac = self.alphas_cumprod.float()[int(self.timesteps[t_start])]
        return float(ac ** 0.5), float((1 - ac) ** 0.5)


class EulerDiscreteScheduler(_Base):
    """leading spacing, steps_offset=1, linear sigma interpolation, epsilon prediction."""

    def __init__(self):
        ac = _alphas_cumprod()
        self.all_sigmas = (((1 - ac) / ac) ** 0.5).numpy()
        self.timesteps = None

    def set_timesteps(self, n, device=None):
        self.num_inference_steps = n
        r = self.num_train_timesteps // n
        ts = (np.arange(0, n) * r).round()[::-1].copy().astype(np.float32) + 1
        sig = np.interp(ts, np.arange(0, len(self.all_sigmas)), self.all_sigmas)
        self.sigmas = torch.from_numpy(np.concatenate([sig, [0.0]]).astype(np.float32))
        self.timesteps = torch.from_numpy(ts)
        self._tab = None

    @property
    def init_noise_sigma(self):
        return float((self.sigmas.max() ** 2 + 1) ** 0.5)

    def tables(self):
        if getattr(self, "_tab", None) is None:
            s = self.sigmas.double()
            coef = torch.stack([torch.ones(len(s) - 1, dtype=torch.float64), s[1:] - s[:-1]], 1)
            self._tab = dict(timesteps=self.timesteps.float(), in_scale=(1.0 / (s[:-1] ** 2 + 1).sqrt()).float(),
                             coef=coef.float(), init_noise_sigma=self.init_noise_sigma)
        return self._tab

    def add_noise_coefficients(self, t_start):
        """diffusers EulerDiscreteScheduler.add_noise after set_begin_index(t_start): x + noise * sigmas[t_start] (fp32)"""
        return 1.0, float(self.sigmas[t_start])


# ---------------------------------------------------------------------------------------------------------------------------------
# Multistep and ancestral samplers: the general step (csrc/elementwise.hip EW_CFG_MSTEP)
#
# DPM-Solver++ 2M needs the previous step's data prediction, the SDE variant and Euler ancestral need fresh noise at every step.  All
# of them are still LINEAR in what the step has at hand -- the latents x, the guided prediction eps, one history buffer h and one noise
# row z -- so each reduces to a six-column table (DESIGN.md "six-coefficient step"):
#
#     x' = cx*x + ce*eps + ch*h + cn*z,        h' = hx*x + he*eps
#
# h holds the previous step's x0 = (x - s*eps) / alpha.  One slot is enough for order 2: the update reads x0_{i-1} and forms x0_i from
# (x, eps) itself, and the slot is overwritten with x0_i by the thread that just read it.
class _GeneralStep(_Base):
    """Common host side of the schedulers that step through the six-column table.  tables(t_start) -> the dict of _Base.tables with
    ``coef`` None and ``coef6`` fp32 [n, 6]; the row at t_start is first order (an image-to-image start has no history: diffusers'
    fresh lower_order_nums).  ``step`` / ``scale_model_input`` are stateful, as diffusers' are: they count steps from set_timesteps /
    set_begin_index and keep the previous data prediction."""
    general_step = True
    needs_history = False        # the step reads / writes the history slot
    stochastic = False           # the step reads a noise row

    def set_begin_index(self, t_start=0):
        self._i, self._h = int(t_start), None

    def _reset(self):
        self._tabs = {}
        self.set_begin_index(0)

    def _order(self, i, t_start=0):
        return 1

    def _row(self, i, order):
        """(cx, ce, ch, cn, hx, he) of table row i at that order, python floats from float64 arithmetic"""
        raise NotImplementedError

    def _in_scale(self):
        return None

    def table_f64(self, t_start=0):
        """the six-column table as it is computed, float64 [n, 6]; tables() rounds it to fp32 once"""
        return torch.tensor([self._row(i, self._order(i, int(t_start))) for i in range(self.num_inference_steps)], dtype=torch.float64)

    def tables(self, t_start=0):
        t_start = int(t_start)
        if t_start not in self._tabs:
            self._tabs[t_start] = dict(timesteps=self.timesteps.float(), in_scale=self._in_scale(), coef=None,
                                       coef6=self.table_f64(t_start).float(), init_noise_sigma=float(self.init_noise_sigma))
        return self._tabs[t_start]

    def scale_model_input(self, x, t):
        s = self._in_scale()
        return x if s is None else x * float(s[self._i])

    def step(self, eps, t, x, return_dict=False, generator=None, noise=None, **kw):
        """one host-side step at the scheduler's own step index (t is accepted for the call surface).  A stochastic scheduler takes its
        noise from ``noise`` or draws it from ``generator`` as diffusers does (randn_tensor of the prediction's shape, on the CPU)."""
        i = self._i
        order = 1 if self._h is None else self._order(i)
        cx, ce, ch, cn, hx, he = self._row(i, order)
        wd = torch.float64 if x.dtype == torch.float64 else torch.float32
        xf, ef = x.to(wd), eps.to(wd)
        out = cx * xf + ce * ef
        if self.needs_history and self._h is not None and ch != 0.0:
            out = out + ch * self._h.to(wd)
        if self.stochastic:
            if noise is None:
                from .pipeline import randn_latents
                noise = randn_latents(tuple(x.shape), generator)
            out = out + cn * noise.to(x.device, wd)
        if self.needs_history:
            self._h = hx * xf + he * ef
        self._i = i + 1
        return (out.to(x.dtype),)


class DPMSolverMultistepScheduler(_GeneralStep):
    """DPM-Solver++ (2M by default) and its SDE variant with diffusers 0.30 semantics under the SDXL scheduler config (scaled-linear
    betas, steps_offset = 1, epsilon prediction, final sigma 0, no thresholding).  With sigma the step's sigma, alpha = 1/sqrt(sigma^2
    + 1), s = sigma * alpha, lambda = log(alpha) - log(s), x0 = (x - s_i eps) / alpha_i and h = lambda_{i+1} - lambda_i:

        first order   x' = (s_{i+1}/s_i) x + A x0_i,                                  A = alpha_{i+1} (1 - e^{-h})
        second order  x' = ... + A (x0_i - x0_{i-1}) / (2 r0),                        r0 = (lambda_i - lambda_{i-1}) / h   (midpoint)
        SDE           x' = (s_{i+1}/s_i) e^{-h} x + B x0_i [+ B (x0_i - x0_{i-1}) / (2 r0)] + s_{i+1} sqrt(1 - e^{-2h}) z,
                                                                                      B = alpha_{i+1} (1 - e^{-2h})

    The first step that runs is first order; so is the last table row when euler_at_final, or lower_order_final with fewer than 15
    steps, or the final sigma is zero (always, here).  At the final sigma 0, lambda = +inf: e^{-h} = 0 is taken explicitly and the
    step returns x0."""
    init_noise_sigma = 1.0

    def __init__(self, algorithm_type="dpmsolver++", solver_order=2, solver_type="midpoint", lower_order_final=True, euler_at_final=False,
                 final_sigmas_type="zero", use_karras_sigmas=False, timestep_spacing="leading"):
        if algorithm_type not in ("dpmsolver++", "sde-dpmsolver++"):
            raise NotImplementedError(f"algorithm_type {algorithm_type!r} (dpmsolver++ or sde-dpmsolver++)")
        if solver_order not in (1, 2):
            raise NotImplementedError(f"solver_order {solver_order} (1 or 2)")
        if solver_type != "midpoint":
            raise NotImplementedError(f"solver_type {solver_type!r} (midpoint)")
        if final_sigmas_type != "zero":
            raise NotImplementedError(f"final_sigmas_type {final_sigmas_type!r} (zero)")
        if timestep_spacing not in ("leading", "trailing"):
            raise NotImplementedError(f"timestep_spacing {timestep_spacing!r} (leading or trailing)")
        self.algorithm_type, self.solver_order, self.solver_type = algorithm_type, int(solver_order), solver_type
        self.lower_order_final, self.euler_at_final, self.final_sigmas_type = bool(lower_order_final), bool(euler_at_final), final_sigmas_type
        self.use_karras_sigmas, self.timestep_spacing = bool(use_karras_sigmas), timestep_spacing
        ac = _alphas_cumprod().float()
        self.all_sigmas = (((1 - ac) / ac) ** 0.5).numpy()                    # fp32, as diffusers forms them
        self.stochastic = algorithm_type == "sde-dpmsolver++"
        self.needs_history = self.solver_order == 2
        self.timesteps = None

    def set_timesteps(self, n, device=None):
        self.num_inference_steps = n = int(n)
        N = self.num_train_timesteps
        if self.timestep_spacing == "leading":
            ts = (np.arange(0, n + 1) * (N // (n + 1))).round()[::-1][:-1].copy().astype(np.int64) + 1
        else:
            ts = np.arange(N, 0, -N / n).round().copy().astype(np.int64) - 1
        sig = self.all_sigmas
        if self.use_karras_sigmas:
            # rho = 7 between the last and the first training sigma; timesteps by log-sigma interpolation, rounded
            lo, hi = float(sig[0]), float(sig[-1])
            ramp = np.linspace(0, 1, n)
            ks = (hi ** (1 / 7.0) + ramp * (lo ** (1 / 7.0) - hi ** (1 / 7.0))) ** 7.0
            ls = np.log(sig)
            ts = np.array([self._sigma_to_t(s, ls) for s in ks]).round().astype(np.int64)
            sigmas = ks
        else:
            sigmas = np.interp(ts, np.arange(0, len(sig)), sig)
        self.sigmas = torch.from_numpy(np.concatenate([sigmas, [0.0]]).astype(np.float32))
        self.timesteps = torch.from_numpy(ts)
        self._reset()

    @staticmethod
    def _sigma_to_t(sigma, log_sigmas):
        ls = np.log(np.maximum(sigma, 1e-10))
        d = ls - log_sigmas
        low = int(np.clip(np.cumsum(d >= 0).argmax(), None, len(log_sigmas) - 2))
        w = np.clip((log_sigmas[low] - ls) / (log_sigmas[low] - log_sigmas[low + 1]), 0, 1)
        return (1 - w) * low + w * (low + 1)

    @staticmethod
    def _asl(sigma):
        """(alpha, s, lambda) of one sigma in float64; lambda = +inf at sigma 0"""
        a = 1.0 / np.sqrt(sigma * sigma + 1.0)
        s = sigma * a
        return a, s, (np.log(a) - np.log(s) if sigma > 0 else np.inf)

    def _order(self, i, t_start=0):
        n = self.num_inference_steps
        if self.solver_order == 1 or i == t_start or i == 0:          # (rows before t_start are never read: they stay as t_start = 0 has them)
            return 1
        if i == n - 1 and (self.euler_at_final or (self.lower_order_final and n < 15) or self.final_sigmas_type == "zero"):
            return 1
        return 2

    def _row(self, i, order):
        sg = self.sigmas.double().numpy()
        a0, s0, l0 = self._asl(sg[i])
        a1, s1, l1 = self._asl(sg[i + 1])
        final = not np.isfinite(l1)
        h = l1 - l0
        if self.stochastic:
            keep = 0.0 if final else np.exp(-h)                       # e^{-h}
            gain = 1.0 if final else -np.expm1(-2.0 * h)              # 1 - e^{-2h}
            base, A, cn = (s1 / s0) * keep, a1 * gain, s1 * np.sqrt(gain)
        else:
            base, A, cn = s1 / s0, a1 * (1.0 if final else -np.expm1(-h)), 0.0
        k = 0.0
        if order == 2:
            if final or i == 0:
                raise ValueError("a second-order row needs a finite step and a previous row")
            k = 0.5 * h / (l0 - self._asl(sg[i - 1])[2])             # 1 / (2 r0)
        return (float(base + A * (1.0 + k) / a0), float(-A * (1.0 + k) * s0 / a0), float(-A * k), float(cn), float(1.0 / a0), float(-s0 / a0))

    def add_noise_coefficients(self, t_start):
        """diffusers DPMSolverMultistepScheduler.add_noise after set_begin_index(t_start): alpha x + s noise at sigmas[t_start]"""
        a, s, _ = self._asl(float(self.sigmas[t_start]))
        return float(a), float(s)


class EulerAncestralDiscreteScheduler(_GeneralStep):
    """"Euler a" with diffusers 0.30 semantics; timesteps, sigmas, input scale and init_noise_sigma as EulerDiscreteScheduler.
        sigma_up = sqrt(sigma_{i+1}^2 (sigma_i^2 - sigma_{i+1}^2) / sigma_i^2),  sigma_down = sqrt(sigma_{i+1}^2 - sigma_up^2)
        x' = x + (sigma_down - sigma_i) eps + sigma_up z"""
    stochastic = True

    def __init__(self):
        self._euler = EulerDiscreteScheduler()
        self.timesteps = None

    def set_timesteps(self, n, device=None):
        self._euler.set_timesteps(n)
        self.num_inference_steps = int(n)
        self.sigmas, self.timesteps = self._euler.sigmas, self._euler.timesteps
        self._reset()

    @property
    def init_noise_sigma(self):
        return self._euler.init_noise_sigma

    def _in_scale(self):
        return self._euler.tables()["in_scale"]

    def _row(self, i, order):
        s = self.sigmas.double()
        s0, s1 = float(s[i]), float(s[i + 1])
        up = (s1 * s1 * (s0 * s0 - s1 * s1) / (s0 * s0)) ** 0.5
        down = (s1 * s1 - up * up) ** 0.5
        return (1.0, down - s0, 0.0, up, 0.0, 0.0)

    def add_noise_coefficients(self, t_start):
        """diffusers EulerAncestralDiscreteScheduler.add_noise after set_begin_index(t_start): x + noise * sigmas[t_start]"""
        return 1.0, float(self.sigmas[t_start])
