"""tests/guarded.py on CPU tensors: the arena that the guarded-placement GPU tests (test_gpu_guarded_ops.py) trust must itself place
views where it says, notice one stray element on either side of a view or inside a row gap, name the allocation and the side, and keep
its guard-size rule at the widest row the GPU file uses."""
import pytest
import torch

import guarded
from guarded import Arena, GuardDamage

MIB = 1 << 20


def _arena(n=8 * MIB):
    return Arena("cpu", n)


def test_carves_are_aligned_strided_and_recorded():
    a = _arena(16 * MIB)
    v0 = a.carve((5, 24), torch.bfloat16)
    v1 = a.carve((3, 7, 24), torch.float16, ld=40)
    v2 = a.carve((3,), torch.float32)
    v3 = a.carve((1001,), torch.uint8, role="scratch")
    v4 = a.carve((1,), torch.int32)
    for v in (v0, v1, v2, v3, v4):
        assert v.data_ptr() % 256 == 0
    assert v0.is_contiguous() and v0.shape == (5, 24)
    assert v1.shape == (3, 7, 24) and v1.stride() == (7 * 40, 40, 1)
    assert v1.view(21, 24).stride() == (40, 1)                    # the token-major [rows, C] view the wrappers take
    assert [c["role"] for c in a.carves] == ["out", "out", "out", "scratch", "out"] and len(a.carves) == 5
    base = a.mem.data_ptr()
    for prev, c in zip(a.carves, a.carves[1:]):
        assert c["off"] - prev["end"] >= max(guarded.guard_bytes(prev["pitch"]), guarded.guard_bytes(c["pitch"]))
    assert a.carves[0]["off"] >= MIB and a.mem.numel() - a.carves[-1]["end"] >= MIB
    assert v1.data_ptr() == base + a.carves[1]["off"]
    with pytest.raises(ValueError):
        a.carve((2, 8), torch.float32, ld=4)
    with pytest.raises(MemoryError):
        a.carve((4 * MIB, 2), torch.float32)


def test_size_for_is_the_layout_carve_produces():
    specs = [((130, 72), torch.bfloat16, 200), ((7,), torch.float32, None), ((2, 9, 40), torch.float32, 48), ((12345,), torch.uint8, None)]
    a = Arena("cpu", Arena.size_for(specs))
    for s in specs:
        a.carve(*s)
    with pytest.raises(MemoryError):                              # exactly enough: one more view does not fit
        a.carve((8,), torch.float32)


def test_sentinel_reads_as_nan_in_every_width():
    a = _arena(4 * MIB)
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        assert torch.isnan(a.mem.view(dt)).all(), dt
    assert (a.mem.view(torch.int16) == guarded.SENTINEL_I16).all()
    assert (a.mem.view(torch.int32) < 0).all()                   # a step counter read from a guard is no valid index
    w = a.mem.view(torch.int32)[0].item() & 0xFFFFFFFF
    assert w == 0xFFA5FFA5
    # ... and an output the op never wrote is caught by the finite check
    a.carve((4, 8), torch.bfloat16)
    with pytest.raises(GuardDamage, match="not finite"):
        a.check()


def test_in_range_writes_pass():
    a = _arena(16 * MIB)
    x = a.place(torch.randn(9, 24).to(torch.bfloat16), ld=56)
    y = a.carve((9, 24), torch.bfloat16, ld=32)
    z = a.carve((2, 3, 5), torch.float32)
    s = a.carve((1,), torch.int32)
    ws = a.carve((1000,), torch.uint8, role="scratch")
    y.copy_(x * 2)
    z.fill_(1.0)
    s.fill_(3)
    ws[:17] = 0                                                   # a workspace may be left half written
    a.check()
    assert torch.equal(y, (x * 2))
    raw = torch.as_strided(x, (9, 56), (56, 1))[:-1, 24:]         # the input's row gaps keep the sentinel
    assert torch.isnan(raw).all()


def test_written_names_a_touched_output_and_reset_starts_over():
    """what the refusal checks of test_gpu_dispatch_contract.py stand on: an untouched output reads as untouched, one written element of an
    output / workspace is named, inputs and sealed outputs of earlier launches do not count, reset() gives the arena back as constructed"""
    a = _arena(16 * MIB)
    a.place(torch.randn(4, 8))
    pre = a.carve((4, 8), torch.float32)                          # written by an earlier launch, then an operand
    pre.fill_(1.0)
    a.seal()
    assert [c["role"] for c in a.carves] == ["in", "in"]
    y = a.carve((9, 24), torch.bfloat16, ld=32)
    ws = a.carve((2, 4096), torch.uint8, role="scratch")
    assert a.written() is None
    y[8, 23] = 0.5
    assert a.written() == a.carves[2]["name"]
    a.reset()
    assert a.carves == [] and (a.mem.view(torch.int16) == guarded.SENTINEL_I16).all()
    a.place(torch.randn(4, 8))
    a.carve((9, 24), torch.bfloat16, ld=32)
    ws = a.carve((2, 4096), torch.uint8, role="scratch")
    assert a.carves[0]["off"] >= MIB and a.written() is None      # the layout starts from the front again
    ws[1, 4095] = 0
    assert a.written() == a.carves[2]["name"] and not a.damage()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32, torch.int32])
@pytest.mark.parametrize("side", ["before", "after", "row gap"])
def test_one_stray_element_is_found_and_named(dtype, side):
    a = _arena(16 * MIB)
    a.place(torch.ones(4, 8, dtype=dtype), name="left neighbour")
    v = a.carve((6, 10), dtype, ld=16, name="victim")
    a.place(torch.ones(4, 8, dtype=dtype), name="right neighbour")
    v.fill_(1)
    a.check()
    es = v.element_size()
    wide = torch.as_strided(v, (6, 16), (16, 1))
    if side == "before":
        torch.as_strided(v, (1,), (1,), v.storage_offset() - 1).fill_(2)
        first = -es
    elif side == "after":
        torch.as_strided(v, (1,), (1,), v.storage_offset() + 5 * 16 + 10).fill_(2)
        first = (5 * 16 + 10) * es
    else:
        wide[2, 10] = 2
        first = (2 * 16 + 10) * es
    with pytest.raises(GuardDamage) as e:
        a.check()
    msg = str(e.value)
    assert f"victim: {side}, bytes [{first}, {first + es - 1}]" in msg, msg
    assert "neighbour" not in msg
    assert a.damage() == [("victim", side, first, first + es - 1)]


def test_slack_up_to_the_next_boundary_is_guarded():
    a = _arena(4 * MIB)
    v = a.carve((3,), torch.bfloat16)                              # 6 bytes: 250 bytes of slack before the next 256-byte boundary
    v.fill_(0)
    a.mem[a.carves[0]["end"] + 200] = 0
    with pytest.raises(GuardDamage, match=r"after, bytes \[206, 206\]"):
        a.check()


def test_guard_rule_at_the_widest_pitch_of_the_gpu_file():
    """guard >= max(1 MiB, 320 rows x pitch): the tallest tile (256 rows) plus one key tile of rows of ANY view fit in its guard"""
    import test_gpu_guarded_ops as G
    pitch = G.MAX_ROW_PITCH_BYTES
    assert pitch >= 4096 * 4                                       # the fp32 softmax rows / the 4096-wide LayerNorm rows
    assert guarded.guard_bytes(pitch) >= max(MIB, 320 * pitch)
    assert guarded.guard_bytes(64) == MIB
    cols = pitch // 2
    a = Arena("cpu", Arena.size_for([((2, cols), torch.bfloat16, None)] * 2))
    a.carve((2, cols), torch.bfloat16)
    a.carve((2, cols), torch.bfloat16)
    c0, c1 = a.carves
    assert c0["off"] >= 320 * pitch and c1["off"] - c0["end"] >= 320 * pitch and a.mem.numel() - c1["end"] >= 320 * pitch
