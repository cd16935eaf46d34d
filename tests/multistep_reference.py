"""Test-local sequential restatement of the multistep and ancestral samplers (diffusers 0.30.0 semantics, recalled from the published
sources; diffusers itself is not installed): DPMSolverMultistepScheduler (dpmsolver++ / sde-dpmsolver++, midpoint, orders 1 and 2,
final sigma zero) and EulerAncestralDiscreteScheduler under the SDXL scheduler config.

Written independently of the product's table form: a stateful ``step`` that keeps a ``model_outputs`` list and a ``lower_order_nums``
counter and evaluates the update formulas literally, in the dtype it is given (float64 latents -> float64 throughout; anything else ->
float32, as diffusers computes).  It imports nothing from the product.  The ``set_timesteps / timesteps / init_noise_sigma /
scale_model_input / step`` surface is what oracle.pipeline.denoise calls.

``noise``: a tensor whose row r is the noise of schedule step r (the rows the device noise bank holds), so that both sides of a
comparison consume the same numbers; without it a stochastic step draws from ``generator``.
``t_start``: an image-to-image start (get_timesteps + set_begin_index): the loop sees timesteps[t_start:], the step index begins at
t_start, nothing is in ``model_outputs``, and the caller's latents are already noised (init_noise_sigma = 1).

A plain helper module; no fixtures, no pytest settings."""
import numpy as np
import torch


def train_sigmas():
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float32) ** 2
    ac = torch.cumprod(1.0 - betas, dim=0)
    return (((1 - ac) / ac) ** 0.5).numpy()                 # float32


def _work_dtype(x):
    return torch.float64 if x.dtype == torch.float64 else torch.float32


class RefDPMSolverMultistep:
    order = 1

    def __init__(self, algorithm_type="dpmsolver++", solver_order=2, lower_order_final=True, euler_at_final=False,
                 use_karras_sigmas=False, timestep_spacing="leading", t_start=0, noise=None, generator=None):
        self.algorithm_type, self.solver_order = algorithm_type, solver_order
        self.lower_order_final, self.euler_at_final = lower_order_final, euler_at_final
        self.use_karras_sigmas, self.timestep_spacing = use_karras_sigmas, timestep_spacing
        self.t_start, self.noise, self.generator = t_start, noise, generator
        self.init_noise_sigma = 1.0

    def set_timesteps(self, n, device=None):
        sig = train_sigmas()
        if self.timestep_spacing == "leading":
            ratio = 1000 // (n + 1)
            ts = (np.arange(0, n + 1) * ratio).round()[::-1][:-1].copy().astype(np.int64)
            ts += 1                                                        # steps_offset
        else:
            ts = np.arange(1000, 0, -(1000 / n)).round().copy().astype(np.int64)
            ts -= 1
        if self.use_karras_sigmas:
            log_sigmas = np.log(sig)
            flipped = np.flip(sig).copy()
            smin, smax = flipped[-1].item(), flipped[0].item()
            rho = 7.0
            ramp = np.linspace(0, 1, n)
            sigmas = (smax ** (1 / rho) + ramp * (smin ** (1 / rho) - smax ** (1 / rho))) ** rho
            # _sigma_to_t over all sigmas at once
            ls = np.log(np.maximum(sigmas, 1e-10))
            dists = ls - log_sigmas[:, np.newaxis]
            low = np.cumsum((dists >= 0), axis=0).argmax(axis=0).clip(max=log_sigmas.shape[0] - 2)
            high = low + 1
            w = ((log_sigmas[low] - ls) / (log_sigmas[low] - log_sigmas[high])).clip(0, 1)
            ts = ((1 - w) * low + w * high).round().astype(np.int64)
        else:
            sigmas = np.interp(ts, np.arange(0, len(sig)), sig)
        self.sigmas = torch.from_numpy(np.concatenate([sigmas, [0.0]]).astype(np.float32))
        self.all_timesteps = torch.from_numpy(ts)
        self.timesteps = self.all_timesteps[self.t_start:]
        self.step_index = self.t_start
        self.model_outputs = [None] * self.solver_order
        self.lower_order_nums = 0

    def scale_model_input(self, x, t):
        return x

    @staticmethod
    def _alpha_sigma(sigma):
        alpha_t = 1 / ((sigma ** 2 + 1) ** 0.5)
        return alpha_t, sigma * alpha_t

    def _noise(self, x):
        if self.noise is not None:
            return self.noise[self.step_index]
        return torch.randn(x.shape, generator=self.generator, dtype=torch.float32)

    def step(self, eps, t, x, return_dict=False, **kw):
        dt = _work_dtype(x)
        i = self.step_index
        n = len(self.all_timesteps)
        sig = self.sigmas.to(dt)
        x, eps = x.to(dt), eps.to(dt)
        # convert_model_output: epsilon prediction -> data prediction
        alpha_s0, sigma_s0 = self._alpha_sigma(sig[i])
        x0 = (x - sigma_s0 * eps) / alpha_s0
        for k in range(self.solver_order - 1):
            self.model_outputs[k] = self.model_outputs[k + 1]
        self.model_outputs[-1] = x0
        final = i == n - 1 and (self.euler_at_final or (self.lower_order_final and n < 15) or True)      # final_sigmas_type == "zero"
        alpha_t, sigma_t = self._alpha_sigma(sig[i + 1])
        lambda_t = torch.log(alpha_t) - torch.log(sigma_t)
        lambda_s0 = torch.log(alpha_s0) - torch.log(sigma_s0)
        h = lambda_t - lambda_s0
        sde = self.algorithm_type == "sde-dpmsolver++"
        z = self._noise(x).to(dt) if sde else None
        if self.solver_order == 1 or self.lower_order_nums < 1 or final:
            if sde:
                out = (sigma_t / sigma_s0 * torch.exp(-h)) * x + (alpha_t * (1 - torch.exp(-2.0 * h))) * x0 \
                    + sigma_t * torch.sqrt(1.0 - torch.exp(-2.0 * h)) * z
            else:
                out = (sigma_t / sigma_s0) * x - (alpha_t * (torch.exp(-h) - 1.0)) * x0
        else:
            m0, m1 = self.model_outputs[-1], self.model_outputs[-2]
            alpha_s1, sigma_s1 = self._alpha_sigma(sig[i - 1])
            lambda_s1 = torch.log(alpha_s1) - torch.log(sigma_s1)
            h_0 = lambda_s0 - lambda_s1
            r0 = h_0 / h
            D0, D1 = m0, (1.0 / r0) * (m0 - m1)
            if sde:
                out = (sigma_t / sigma_s0 * torch.exp(-h)) * x + (alpha_t * (1 - torch.exp(-2.0 * h))) * D0 \
                    + 0.5 * (alpha_t * (1 - torch.exp(-2.0 * h))) * D1 + sigma_t * torch.sqrt(1.0 - torch.exp(-2.0 * h)) * z
            else:
                out = (sigma_t / sigma_s0) * x - (alpha_t * (torch.exp(-h) - 1.0)) * D0 - 0.5 * (alpha_t * (torch.exp(-h) - 1.0)) * D1
        if self.lower_order_nums < self.solver_order:
            self.lower_order_nums += 1
        self.step_index += 1
        return (out,)


class RefEulerAncestral:
    order = 1

    def __init__(self, t_start=0, noise=None, generator=None):
        self.t_start, self.noise, self.generator = t_start, noise, generator

    def set_timesteps(self, n, device=None):
        # sigmas as the project's EulerDiscrete forms them: from the fp32 alphas_cumprod, in float64
        betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float32) ** 2
        ac = torch.cumprod(1.0 - betas, dim=0).double()
        sig = (((1 - ac) / ac) ** 0.5).numpy()
        ts = (np.arange(0, n) * (1000 // n)).round()[::-1].copy().astype(np.float32)
        ts += 1
        sigmas = np.interp(ts, np.arange(0, len(sig)), sig)
        self.sigmas = torch.from_numpy(np.concatenate([sigmas, [0.0]]).astype(np.float32))
        self.all_timesteps = torch.from_numpy(ts)
        self.timesteps = self.all_timesteps[self.t_start:]
        self.step_index = self.t_start

    @property
    def init_noise_sigma(self):
        return 1.0 if self.t_start else float((self.sigmas.max() ** 2 + 1) ** 0.5)

    def scale_model_input(self, x, t):
        sigma = self.sigmas[self.step_index].to(_work_dtype(x))
        return x / ((sigma ** 2 + 1) ** 0.5)

    def step(self, eps, t, x, return_dict=False, **kw):
        dt = _work_dtype(x)
        i = self.step_index
        sig = self.sigmas.to(dt)
        x, eps = x.to(dt), eps.to(dt)
        sigma = sig[i]
        pred_original_sample = x - sigma * eps
        sigma_from, sigma_to = sig[i], sig[i + 1]
        sigma_up = (sigma_to ** 2 * (sigma_from ** 2 - sigma_to ** 2) / sigma_from ** 2) ** 0.5
        sigma_down = (sigma_to ** 2 - sigma_up ** 2) ** 0.5
        derivative = (x - pred_original_sample) / sigma
        z = self.noise[i] if self.noise is not None else torch.randn(x.shape, generator=self.generator, dtype=torch.float32)
        out = x + derivative * (sigma_down - sigma) + z.to(dt) * sigma_up
        self.step_index += 1
        return (out,)
