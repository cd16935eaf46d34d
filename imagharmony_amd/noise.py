"""The seeded step noise, restated in numpy (include/imh.h "seeded step noise" is the specification; csrc/imh_philox.h the product's code).

The noise a stochastic sampler adds at a step is a pure function of (seed, lane, table row, stream, element): Philox4x32-10 as published
(Salmon et al., Random123) on the counter (element >> 2, row, stream, lane) under the key (seed & 0xffffffff, seed >> 32); the four words
become four uniforms u = ((w >> 9) + 0.5) * 2^-23 and, by Box-Muller, four normals; element e takes the (e & 3)-th.  Here the words are
exact and the normals are computed in float64 and rounded to fp32 once -- the yardstick the kernels are held against."""
import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
_SH = np.uint64(32)


def check_seed(seed):
    """a seed is an integer in [0, 2**64); anything else is a ValueError"""
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
        raise ValueError(f"seed {seed!r} is not an integer")
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"seed {seed} outside [0, 2**64)")
    return seed


def seed_rows(seeds, lanes=None):
    """uint32 [S, 4]: row s = (seed & 0xffffffff, seed >> 32, lane, 0).  lanes None: 0 for every sample (each has a seed of its own);
    one seed serving a batch passes the sample indices."""
    seeds = [check_seed(s) for s in seeds]
    if lanes is None:
        lanes = [0] * len(seeds)
    lanes = [int(l) for l in lanes]
    if len(lanes) != len(seeds):
        raise ValueError(f"{len(lanes)} lanes for {len(seeds)} seeds")
    if any(not 0 <= l < 2 ** 32 for l in lanes):
        raise ValueError(f"lanes {lanes} outside [0, 2**32)")
    return np.array([[s & 0xFFFFFFFF, s >> 32, l, 0] for s, l in zip(seeds, lanes)], dtype=np.uint32).reshape(len(seeds), 4)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (broadcastable), key: two uint32 scalars / arrays -> four uint32 arrays"""
    c = [np.asarray(x, dtype=np.uint64) for x in np.broadcast_arrays(*[np.asarray(v, dtype=np.uint64) for v in counter])]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]                       # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> _SH) ^ c[1] ^ np.uint64(k0), p1 & _MASK, (p0 >> _SH) ^ c[3] ^ np.uint64(k1), p0 & _MASK]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def seeded_words(seeds, row, shape, lanes=None, stream=0):
    """uint32 [S, *shape]: the raw words, sample s from seeds[s] / lanes[s]; prod(shape) must be a multiple of 4"""
    rows = seed_rows(seeds, lanes)
    n = int(np.prod(shape))
    if n % 4 or n <= 0:
        raise ValueError(f"a sample of {n} elements is not a whole number of quads")
    if not 0 <= int(row) < 2 ** 32 or not 0 <= int(stream) < 2 ** 32:
        raise ValueError(f"row {row} / stream {stream} outside [0, 2**32)")
    quad = np.arange(n // 4, dtype=np.uint64)
    out = np.empty((len(rows), n), dtype=np.uint32)
    for s, (k0, k1, lane, _) in enumerate(rows):
        w = philox4x32_10((quad, int(row), int(stream), int(lane)), (k0, k1))
        out[s] = np.stack(w, 1).reshape(-1)
    return out.reshape((len(rows),) + tuple(int(d) for d in shape))


def normals_from_words(words, dtype=np.float32):
    """Box-Muller over quads of words (last axis flattened per sample): float64 arithmetic, rounded once to ``dtype``"""
    w = np.asarray(words, dtype=np.uint32)
    q = w.reshape(w.shape[0], -1, 4)
    u = ((q >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    z = np.empty_like(u)
    for a in (0, 2):
        rho, ang = np.sqrt(-2.0 * np.log(u[..., a])), 2.0 * np.pi * u[..., a + 1]
        z[..., a], z[..., a + 1] = rho * np.cos(ang), rho * np.sin(ang)
    return z.reshape(w.shape).astype(dtype)


def seeded_randn(seeds, row, shape, lanes=None, stream=0, dtype=np.float32):
    """[S, *shape] normals of table row ``row``: what the seeded step adds (times cn) to sample s's latent of ``shape`` (4, H, W)"""
    return normals_from_words(seeded_words(seeds, row, shape, lanes, stream), dtype)
