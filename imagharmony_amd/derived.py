"""The one cache of derived weights: every packed, padded, phase-summed, interleaved, stacked or LayerNorm-folded copy of a parameter.

The contract, stated once.  A copy lives on the module that owns its sources, as ``(key, value)`` in one attribute, and is found again
by its key: ``(data_ptr, _version)`` of every source tensor, plus whatever else the built value depends on -- the target dtype / device
(``where``) and the builder's own arguments (``extra``: a pad width, a flag).  So a copy is rebuilt after ``load_state_dict`` or
``weight.copy_`` (in place: the address stays, the version moves), after ``.to()`` or a re-assigned parameter (the address moves), and
for another dtype, device or extra.  A store that goes behind torch's back moves neither: who writes a weight from a kernel bumps its
version too (``lora.LoRAState.apply``: ``torch.autograd.graph.increment_version``).

A rebuilt copy is a NEW tensor.  A recorded plan (Ctx(record=True), a captured hipGraph) holds pointers into the copies it was recorded
with, so whoever changes a weight must re-record: DenoiseEngine keys its plans by ``unet.lora_epoch``, the CLIP towers drop their plans
with their copies (clip_tower.Tower.derived), and ``modules.Graphed`` says in its docstring why it wraps only modules that derive nothing.
"""


def vkey(*tensors):
    """storage address AND in-place version counter per source tensor (None for a source that is not there, e.g. a missing bias): the
    only place in the package that reads ``_version`` to key a copy of a weight"""
    return tuple((t.data_ptr(), t._version) if t is not None else None for t in tensors)


def derived(holder, slot, srcs, build, where=(), extra=()):
    """``holder.<slot>``'s value while its key holds, else ``build()`` (a tensor or a tuple of them), stored there and returned.
    srcs: EVERY tensor build() reads; where: the target dtype and device (``ctx.dtype, str(ctx.device)``), or what of them applies;
    extra: further arguments of build().  where and extra are compared with ``==``, item by item."""
    key = (vkey(*srcs), tuple(where), tuple(extra))
    c = getattr(holder, slot, None)
    if c is None or c[0] != key:
        c = (key, build())
        setattr(holder, slot, c)
    return c[1]
