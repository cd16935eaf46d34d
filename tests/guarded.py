"""Guarded placement of kernel operands: every input and output of an op is a view into ONE allocation filled with a NaN
sentinel, with a wide guard band on either side and (optionally) a row pitch wider than the row.  After the op, check() proves that
no byte outside the carved regions changed and that the outputs are finite -- a store past a ragged edge tile lands in a guard, a
load past the operand that reaches a result turns it into NaN (or changes its bits against the densely placed run).

What this cannot see: a load outside the operand whose value is discarded (a masked lane, an unstored accumulator row).  The guard
bands are sized so that such a stray access of a whole tile still lands inside the arena: the tests observe an overrun, they can
never cause a fault.

A plain helper module (imported by tests/test_guarded_host.py and tests/test_gpu_guarded_ops.py); no fixtures, no pytest settings."""
import torch

from imagharmony_amd.ctx import Ctx

ALIGN = 256                     # every view starts on a 256-byte boundary (what Ctx.new's pool blocks guarantee)
GUARD_MIN = 1 << 20             # guard band: at least 1 MiB ...
GUARD_ROWS = 320                # ... and at least 320 rows of the view's pitch: the tallest tile (256 rows) plus one key tile (64)
# the sentinel: the two bytes A5 FF repeated.  Read as 16 bits it is 0xFFA5 (bf16 and fp16: exponent all ones, mantissa != 0), as
# 32 bits 0xFFA5FFA5 -- a NaN in every float format the kernels use, with a payload that stale pool memory does not hold; as int32
# it is a large negative number (an index read from a guard does not pass for a step)
SENTINEL = (0xA5, 0xFF)
SENTINEL_I16 = -91              # 0xFFA5 as int16


def _align(n, a=ALIGN):
    return (n + a - 1) // a * a


def _esize(dtype):
    return torch.empty((), dtype=dtype).element_size()


def _geometry(shape, dtype, ld):
    """(rows, row bytes, pitch bytes, extent bytes) of a view whose last dim is the row and whose rows are ld elements apart"""
    shape = tuple(int(s) for s in shape)
    es = _esize(dtype)
    cols = shape[-1] if shape else 1
    rows = 1
    for s in shape[:-1]:
        rows *= s
    ld = cols if ld is None else int(ld)
    if ld < cols:
        raise ValueError(f"leading dimension {ld} is narrower than the row ({cols})")
    return rows, cols * es, ld * es, ((rows - 1) * ld + cols) * es if rows > 0 else 0


def guard_bytes(pitch_bytes):
    return max(GUARD_MIN, GUARD_ROWS * int(pitch_bytes))


class GuardDamage(AssertionError):
    pass


class Arena:
    """One allocation of nbytes on device, sentinel-filled; carve() hands out guarded views of it and check() audits the rest."""

    def __init__(self, device, nbytes):
        nbytes = _align(int(nbytes)) + ALIGN
        self.raw = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.skew = (-self.raw.data_ptr()) % ALIGN            # offset of the first 256-byte boundary inside the allocation
        self.mem = self.raw[self.skew:self.skew + nbytes - ALIGN]
        self.mem.view(torch.int16).fill_(SENTINEL_I16)
        self.device = self.raw.device
        self.carves = []            # dicts: name, role, off, rows, rowb, pitch, end, guard, view
        self._end = 0               # end of the last carve
        self._guard = 0             # its guard

    def reset(self):
        """the arena as constructed: the sentinel everywhere, no carves (views handed out before are dead)"""
        self.mem.view(torch.int16).fill_(SENTINEL_I16)
        self.carves, self._end, self._guard = [], 0, 0

    def seal(self):
        """every "out" carve so far becomes an "in": what earlier launches wrote are operands of the launch that follows, so that
        written() speaks of that launch's own outputs"""
        for c in self.carves:
            if c["role"] == "out":
                c["role"] = "in"

    def written(self):
        """name of the first carve other than an input ("out" / "scratch") that no longer holds the sentinel bit for bit, else None --
        for a refused launch: it must have left its outputs, side outputs and workspaces untouched"""
        pat = torch.tensor(SENTINEL, dtype=torch.uint8, device=self.device)
        for c in self.carves:
            if c["role"] != "in" and c["end"] > c["off"] and bool((self.mem[c["off"]:c["end"]].view(-1, 2) != pat).any()):
                return c["name"]
        return None

    # -------------------------------------------------------------------------------------------- layout
    @staticmethod
    def _next(end, prev_guard, pitch):
        """offset of a new view behind a carve that ended at `end`: both neighbours' guards are honoured"""
        g = guard_bytes(pitch)
        return _align(end + max(prev_guard, g)), g

    @classmethod
    def size_for(cls, specs):
        """bytes an arena needs for the carves specs = [(shape, dtype, ld), ...] in that order (the layout carve() produces)"""
        end, guard = 0, 0
        for shape, dtype, ld in specs:
            _, _, pitch, extent = _geometry(shape, dtype, ld)
            off, guard = cls._next(end, guard, pitch)
            end = off + extent
        return _align(end + max(guard, GUARD_MIN))

    def carve(self, shape, dtype, ld=None, role="out", name=None):
        """a view of `shape` (rows = all dims but the last, ld elements apart) starting on a 256-byte boundary, a guard band of
        max(1 MiB, 320 rows x pitch) before and after it.  role: "out" (check() wants it finite), "in" (place()), "scratch" (a
        workspace: the op may leave any bits in it)"""
        if isinstance(shape, int):
            shape = (shape,)
        shape = tuple(int(s) for s in shape)
        rows, rowb, pitch, extent = _geometry(shape, dtype, ld)
        off, g = self._next(self._end, self._guard, pitch)
        if off + extent + g > self.mem.numel():
            raise MemoryError(f"arena of {self.mem.numel()} bytes cannot hold {shape} {dtype} (ld {ld}) with its guards at offset {off}")
        cols = shape[-1] if shape else 1
        ldv = cols if ld is None else int(ld)
        flat = self.mem[off:off + extent].view(dtype)
        if rows * cols == 0 or ldv == cols:
            view = flat[:rows * cols].view(shape)
        else:
            view = torch.as_strided(flat, (rows, cols), (ldv, 1)).unflatten(0, shape[:-1]) if len(shape) > 1 else flat[:cols]
        self.carves.append(dict(name=name or f"#{len(self.carves)} {role} {shape} {str(dtype).replace('torch.', '')}" + (f" ld={ldv}" if ldv != cols else ""),
                                role=role, off=off, rows=rows, rowb=rowb, pitch=pitch, end=off + extent, guard=g, view=view))
        self._end, self._guard = off + extent, g
        assert view.data_ptr() % ALIGN == 0
        return view

    def place(self, t, ld=None, name=None):
        """carve a view for the input t and copy it in; guards and row gaps keep the sentinel"""
        v = self.carve(tuple(t.shape), t.dtype, ld=ld, role="in", name=name)
        v.copy_(t)
        return v

    # -------------------------------------------------------------------------------------------- audit
    def _damage_mask(self):
        """bool per byte of the arena: differs from the sentinel AND lies outside every carved row"""
        pat = torch.tensor(SENTINEL, dtype=torch.uint8, device=self.device)
        bad = (self.mem.view(-1, 2) != pat).view(-1)
        for c in self.carves:
            if c["rows"] == 0 or c["rowb"] == 0:
                continue
            if c["pitch"] == c["rowb"]:
                bad[c["off"]:c["end"]] = False
            else:
                span = bad[c["off"]:c["off"] + (c["rows"] - 1) * c["pitch"]].view(c["rows"] - 1, c["pitch"]) if c["rows"] > 1 else None
                if span is not None:
                    span[:, :c["rowb"]] = False
                bad[c["end"] - c["rowb"]:c["end"]] = False
        return bad

    def damage(self):
        """[(allocation name, side, first byte, last byte)] with side in before / after / row gap and byte offsets relative to the
        view's first byte; empty when every guard is intact"""
        bad = self._damage_mask()
        if not bool(bad.any()):
            return []
        found = []
        n = bad.numel()
        for i, c in enumerate(self.carves):
            lo = self.carves[i - 1]["end"] if i else 0
            hi = self.carves[i + 1]["off"] if i + 1 < len(self.carves) else n
            mid_lo = (lo + c["off"]) // 2 if i else 0           # the band between two views is split: each half named after its neighbour
            mid_hi = (c["end"] + hi) // 2 if i + 1 < len(self.carves) else n
            for side, a, b in (("before", mid_lo, c["off"]), ("row gap", c["off"], c["end"]), ("after", c["end"], mid_hi)):
                if b <= a:
                    continue
                idx = bad[a:b].nonzero()
                if idx.numel():
                    found.append((c["name"], side, int(idx[0]) + a - c["off"], int(idx[-1]) + a - c["off"]))
        return found

    def check(self):
        """raise GuardDamage naming every damaged allocation / side / first and last damaged byte; then require every "out" view to be finite"""
        found = self.damage()
        if found:
            raise GuardDamage("memory outside the operands was written: " + "; ".join(
                f"{name}: {side}, bytes [{first}, {last}] relative to the view" for name, side, first, last in found))
        for c in self.carves:
            v = c["view"]
            if c["role"] == "out" and v.numel() and v.dtype.is_floating_point and not bool(torch.isfinite(v).all()):
                nbad = int((~torch.isfinite(v)).sum())
                raise GuardDamage(f"{c['name']}: {nbad} of {v.numel()} output elements are not finite (sentinel read into a result, or an element never written)")


class GuardCtx(Ctx):
    """a Ctx whose every allocation -- outputs, statistics, partials, tables, temporaries (Ctx.new) and split-K / GroupNorm workspaces
    (Ctx.workspace, at exactly the byte count asked for) -- is a guarded carve of one arena; free() is a no-op (nothing is reused, so
    check() sees every buffer as the op left it).  zero_slab() buffers stay ordinary zero tensors."""

    def __init__(self, arena, dtype=torch.bfloat16):
        super().__init__(arena.device, dtype)
        self.arena = arena

    def new(self, *shape, dtype=None):
        return self.arena.carve(shape, dtype or self.dtype, role="out")

    def workspace(self, nbytes):
        return self.arena.carve((int(nbytes),), torch.uint8, role="scratch")

    def free(self, t):
        pass


class TraceCtx(Ctx):
    """the plain Ctx (pool blocks, 1 MiB workspace slab) that also notes every allocation it is asked for, so that the arena of the
    guarded run of the same op can be sized once, before the run"""

    def __init__(self, device, dtype=torch.bfloat16):
        super().__init__(device, dtype)
        self.specs = []

    def new(self, *shape, dtype=None):
        self.specs.append((tuple(int(s) for s in shape), dtype or self.dtype, None))
        return super().new(*shape, dtype=dtype)

    def workspace(self, nbytes):
        self.specs.append(((int(nbytes),), torch.uint8, None))
        return super().workspace(nbytes)

    # the dense counterparts of Arena.place / Arena.carve: same signature, plain dense tensors
    def put(self, t, ld=None, name=None):
        self.specs.append((tuple(t.shape), t.dtype, ld))
        return t

    def out(self, shape, dtype, ld=None, role="out", name=None):
        if isinstance(shape, int):
            shape = (shape,)
        self.specs.append((tuple(shape), dtype, ld))
        return torch.zeros(tuple(shape), dtype=dtype, device=self.device)


def run_dense_and_guarded(device, dtype, body):
    """body(ctx, put, out) -> tensor or tuple of tensors; put(t, ld=None) hands an input over, out(shape, dtype, ld=None) an output the
    caller allocates.  Runs it once densely (TraceCtx: a plain Ctx) and once under guarded placement (GuardCtx, every put a
    place(), every out a carve(), in an arena sized from the dense run's allocations) -> (dense results, guarded results, arena)."""
    tr = TraceCtx(device, dtype)
    dense = body(tr, tr.put, tr.out)
    arena = Arena(device, Arena.size_for(tr.specs))
    g = GuardCtx(arena, dtype)
    guarded = body(g, arena.place, arena.carve)
    if arena.device.type == "cuda":
        torch.cuda.synchronize(arena.device)
    as_tuple = lambda r: tuple(r) if isinstance(r, (tuple, list)) else (r,)
    return as_tuple(dense), as_tuple(guarded), arena
