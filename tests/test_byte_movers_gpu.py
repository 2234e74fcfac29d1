"""Every word of every byte mover on the device, on every vector width and both trips of the grid-stride loops (cases, oracle and
planted errors: tests/byte_movers_ref.py; what the table covers and what the planted errors change: tests/test_byte_movers_cpu.py).

For each case: every operand the caller supplies is uploaded inside a guarded allocation [guard | payload | guard] whose guards,
and whose payload where it is an output, hold the canary word; the payload starts 16 bytes in (plus the guard the case asks for)
or the case's element offset further.  The leaf ops.tensor_op_plan reports for the real data_ptr()s must be the leaf the table
names; the op runs through its public entry point; every word of every output is compared with the oracle by array_equal on
the storage words; every guard and every input must be unchanged; where the wrapper takes out=, the allocating form must give
the same words.  No mutated kernel runs here: the planted errors live on the CPU."""

from __future__ import annotations

import numpy as np
import pytest

from tests import byte_movers_ref as R

pytestmark = pytest.mark.gpu

pk = pytest.importorskip("pygpukit_amd")
from pygpukit_amd import _hip, ops  # noqa: E402
from pygpukit_amd.core import bfloat16, float16, float32, int32, int64, uint8  # noqa: E402
from pygpukit_amd.core.array import GPUArray  # noqa: E402

DT = {"u8": uint8, "bf16": bfloat16, "f16": float16, "f32": float32, "i64": int64, "i32": int32}
GROUPS = R.groups()


class Operand:
    """One operand inside its guarded allocation: [guard | off elements | payload | guard], the guards whole 16-byte units."""

    def __init__(self, op: R.Op, off: int):
        isz = R.ITEM[op.item]
        self.item, self.shape, self.n = op.item, op.words.shape, int(op.words.size)
        self.pad = -(-(16 + op.guard * isz) // 16) * 16 // isz
        self.at = self.pad + off
        self.sent = R.canary(op.item, (self.at + self.n + self.pad,))
        self.sent[self.at:self.at + self.n] = op.words.reshape(-1)
        self.root = GPUArray((self.sent.size,), DT[op.item])
        self.root.copy_from_numpy(self.sent)
        self.arr = self.root.narrow(self.at, self.n).view(tuple(self.shape))
        assert self.root.data_ptr() % 16 == 0 and self.arr.data_ptr() % 16 == (off * isz) % 16

    def back(self):
        """(words of the payload, True when both guards are untouched) after the call."""
        got = np.ascontiguousarray(self.root.to_numpy()).view(R.WORD[self.item]).reshape(-1)
        inner = slice(self.at, self.at + self.n)
        guards_ok = np.array_equal(got[:inner.start], self.sent[:inner.start]) and np.array_equal(got[inner.stop:], self.sent[inner.stop:])
        return got[inner].reshape(self.shape).copy(), bool(guards_ok)


def words_of(value, item: str, shape) -> np.ndarray:
    """Storage words of what an entry point returned: a GPUArray or a Python int."""
    if isinstance(value, GPUArray):
        assert value.dtype == DT[item] and tuple(value.shape) == tuple(shape), (value.dtype, value.shape, item, shape)
        return np.ascontiguousarray(value.to_numpy()).view(R.WORD[item]).reshape(shape)
    return np.asarray([value]).astype(R.WORD[item]).reshape(shape)


def launch(c: R.Case, a: dict, given: bool = True):
    """Run the entry point.  Returns what it returned where that is the output ("ret" operands, or `given=False`: the allocating
    form of a wrapper that takes out=)."""
    s, e = c.shape, c.extra
    out = {"out": a["out"]} if given and "out" in a else {}
    if c.fam == "transpose":
        if c.entry == "transpose":
            return ops.transpose(a["in"])
        if c.entry == "T":
            return a["in"].T
        return getattr(ops, c.entry)(a["in"], **out)
    if c.fam == "row_map":
        if c.entry == "repeat_interleave_axis1":
            return ops.repeat_interleave_axis1(a["in"], e[0])
        if c.entry == "transpose_102":
            return a["in"].transpose(1, 0, 2)
        return getattr(ops, c.entry)(a["in"], **out)
    if c.fam == "split_qkv":
        return ops.split_qkv_batch(a["qkv"], a["q"], a["k"], a["v"], s[1], s[2], s[3])
    if c.fam == "gather":
        if c.entry == "embedding_lookup":
            return ops.embedding_lookup(a["table"], a["out"], e[0])
        if c.entry == "embedding_lookup_ptr":
            return ops.embedding_lookup_ptr(a["table"], a["out"], a["ids"])
        if c.entry == "embedding_lookup_batch":
            return ops.embedding_lookup_batch(a["table"], a["out"], a["ids"], len(e))
        return ops.gather_embeddings(a["ids"], a["table"], len(e))
    if c.fam == "slice":
        return ops.slice_rows_range_ptr(a["table"], a["out"], a["start"], e[1])
    if c.fam == "kv_write":
        if c.entry == "kv_cache_update_gqa_ptr":
            return ops.kv_cache_update_gqa_ptr(a["new_kv"], a["cache"], e[1], a["pos"])
        return getattr(ops, c.entry)(a["new_kv"], a["cache"], e[1], e[3])
    if c.fam == "seq_copy":
        if c.entry in ("kv_cache_update", "kv_cache_prefill"):
            return getattr(ops, c.entry)(a["new_kv"], a["cache"], e[1])
        if c.entry == "concat_axis0":
            return ops.concat_axis0(a["a"], a["b"])
        if c.entry == "reshape_copy":
            return ops.reshape_copy(a["in"], **out) if given else ops.reshape_copy(a["in"], e)
        return a["in"].reshape(*e)
    if c.fam == "argmax":
        if c.entry in ("argmax", "argmax_int"):
            return getattr(ops, c.entry)(a["x"].view((s[1],)))
        if c.entry == "sample_greedy":
            return ops.sample_greedy(a["x"])
        if c.entry == "argmax_sample":
            return ops.argmax_sample(a["x"], s[0], s[1])
        return ops.argmax_rows(a["x"], **(out if c.entry == "argmax_rows_out" else {}))
    if c.fam == "paged_write":
        return getattr(ops, c.entry)(a["k"], a["v"], a["k_cache"], a["v_cache"], a["slots"])
    if c.fam == "scatter_last":
        return ops.scatter_last_token_logits(a["logits"], a["start"], a["lens"], s[0], s[1], **out)
    if c.fam == "position_ids":
        return ops.prepare_position_ids(a["start"], a["ctx"], a["pf"], a["lens"], s[0], a["total"])
    if c.fam == "check_eos":
        return ops.check_eos(a["tokens"], e[1])
    if c.fam == "cumsum":
        return ops.compute_cumsum(a["in"])
    assert c.fam == "batch_inputs", c.fam
    got, total = ops.prepare_batch_inputs([list(t) for t in e])
    assert total == sum(len(t) for t in e)
    return got


HAS_OUT = ("transpose_3d_012", "transpose_4d_0132", "transpose_3d_021", "transpose_4d_0213", "reshape_copy", "argmax_rows_out", "scatter_last_token_logits")


def run_case(c: R.Case) -> None:
    o = R.operands(c)
    want = R.expected(c, o)
    p = {n: Operand(op, R.off(c, n)) for n, op in o.items() if op.role != "ret"}
    a = {n: q.arr for n, q in p.items()}
    if c.fam == "position_ids":
        a["total"] = int(o["out"].words.size)
    # 1. the leaf, from the real pointers
    args = R.plan_args(c)
    if args is not None:
        op, rows, row_bytes, isz, tested, kw = args
        assert ops.tensor_op_plan(op, rows, row_bytes, isz, [a[n] for n in tested if n in a], **kw) == c.leaf, str(c)
    else:
        assert c.leaf is None
    # 2. run
    ret = launch(c, a)
    # 3. every word of every output, 4. the guards and the inputs
    got = {}
    for n, op in o.items():
        if op.role == "ret":
            got[n] = words_of(ret, op.item, op.words.shape)
            continue
        w, guards_ok = p[n].back()
        assert guards_ok, f"{c}: the guard around {n} was written"
        if op.role == "in":
            assert np.array_equal(w, op.words), f"{c}: input {n} was written"
        else:
            got[n] = w
    assert set(got) == set(want)
    for n in want:
        if not np.array_equal(got[n], want[n]):
            bad = np.flatnonzero(got[n].reshape(-1) != want[n].reshape(-1))
            raise AssertionError(f"{c}: {bad.size} of {want[n].size} words of {n} differ, first at flat index {bad[0]}: "
                                 f"got {got[n].reshape(-1)[bad[0]]:#x}, expected {want[n].reshape(-1)[bad[0]]:#x}")
    # 5. out= against the allocating form, bit for bit
    if c.entry in HAS_OUT:
        assert ret is a["out"]
        twin = launch(c, a, given=False)
        assert twin is not a["out"]
        assert np.array_equal(words_of(twin, o["out"].item, o["out"].words.shape), got["out"]), f"{c}: out= differs from the allocating form"


@pytest.mark.parametrize("key", list(GROUPS), ids=str)
def test_every_word_on_every_width_and_trip(key):
    for c in GROUPS[key]:
        run_case(c)


def test_batches_beyond_65535_are_refused_before_any_launch():
    """gridDim.z carries the batch: transpose_3d_012 / transpose_4d_0132 raise on the host and leave the output as it was."""
    x = Operand(R.Op("u8", np.zeros((65536, 1, 1), np.uint8), "in"), 0)
    y = Operand(R.Op("u8", R.canary("u8", (65536, 1, 1)), "out"), 0)
    with pytest.raises(_hip.PgkError, match="65535"):
        ops.transpose_3d_012(x.arr, out=y.arr)
    with pytest.raises(_hip.PgkError, match="65535"):
        ops.transpose_4d_0132(x.arr.view((256, 256, 1, 1)), out=y.arr.view((256, 256, 1, 1)))
    with pytest.raises(ValueError, match="65535"):
        ops.tensor_op_plan("transpose_batched", 1, 1, 1, batch=65536)
    w, guards_ok = y.back()
    assert guards_ok and (w == R.CANARY["u8"]).all()
    assert ops.tensor_op_grid("transpose_batched", 1, 1, 1, batch=65535) == 65535


def test_scatter_last_token_logits_takes_a_gpt2_vocabulary():
    """50257 words per row: 100514 bytes in float16 (2-byte vectors), 201028 in float32 (4-byte vectors); neither is a multiple of 16."""
    for item, leaf in (("f16", "vec2"), ("f32", "vec4")):
        c = next(c for c in R.CASES if (c.fam, c.item, c.shape) == ("scatter_last", item, (3, 50257)))
        assert c.leaf == leaf and (50257 * R.ITEM[item]) % 16 != 0
        run_case(c)
