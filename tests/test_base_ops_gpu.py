"""Every element of every base op kernel on the device, on every dispatch branch (cases, oracle and bars: tests/base_ops_ref.py;
what the bars admit and reject: tests/test_base_ops_cpu.py).

For each case: every operand is uploaded inside a padded buffer whose padding holds a NaN pattern, 16-byte aligned or one
element past alignment as the case says; the leaf base_op_plan reports for the real pointers (data_ptr() % 16) must be the
leaf the table names; the op runs; every element of every output is compared with the float64 oracle, as storage words or
under the derived bar; the padding on both sides of every operand and every input must be unchanged.  The in-place forms
must equal the out-of-place result bit for bit."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests import base_ops_ref as R

pytestmark = pytest.mark.gpu

pk = pytest.importorskip("pygpukit_amd")
from pygpukit_amd import ops  # noqa: E402
from pygpukit_amd.core import bfloat16, float16, float32, uint8  # noqa: E402
from pygpukit_amd.core.array import GPUArray  # noqa: E402
from pygpukit_amd.ops._common import call  # noqa: E402

DT = {"f32": float32, "f16": float16, "bf16": bfloat16, "u8": uint8}
WORD = {"f32": np.uint32, "f16": np.uint16, "bf16": np.uint16, "u8": np.uint8}
GROUPS = R.groups()


class Operand:
    """One operand inside its guarded buffer: [guard | n elements | guard], the elements starting 16 bytes (aligned) or one
    element (misaligned) into a pool allocation."""

    def __init__(self, words: np.ndarray, dt: str, shape, misaligned: bool):
        pad = 16 // R.ITEM[dt]
        self.dt, self.n, self.off = dt, int(np.prod(shape)), 1 if misaligned else pad
        self.sent = np.full(self.n + 2 * pad, R.GUARD_WORD[dt], WORD[dt])
        self.sent[self.off:self.off + self.n] = np.asarray(words, WORD[dt]).reshape(-1)
        self.root = GPUArray((self.sent.size,), DT[dt])
        self.root.copy_from_numpy(self.sent)
        self.arr = self.root.narrow(self.off, self.n).view(tuple(shape))
        self.shape = tuple(shape)

    def back(self):
        """(words of the elements, True when both guards are untouched) after the call."""
        got = np.ascontiguousarray(self.root.to_numpy()).view(WORD[self.dt]).reshape(-1)
        inner = slice(self.off, self.off + self.n)
        guards_ok = (got[:self.off] == self.sent[:self.off]).all() and (got[inner.stop:] == self.sent[inner.stop:]).all()
        return got[inner].reshape(self.shape).copy(), bool(guards_ok)


def place(c: R.Case) -> dict:
    ins = R.inputs(c)
    placed = {}
    for name, (dt, shape, _) in R.operands(c).items():
        if name in ins:
            words = ins[name] if dt == "u8" else R.to_words(ins[name], dt)
            if dt != "u8":                      # keep the NaN half of the RoPE tables as uploaded: canonical NaN words
                assert (R.from_words(words, dt)[~np.isnan(ins[name])] == ins[name][~np.isnan(ins[name])]).all()
        else:
            words = R.initial_words(c, name)
        placed[name] = Operand(words, dt, shape, name in c.mis)
    return placed


def launch(c: R.Case, p: dict) -> None:
    a = {k: v.arr for k, v in p.items()}
    code = DT[c.dtype].code
    if c.fam == "binary":
        if c.op.endswith("_inplace"):
            getattr(ops, c.op)(a["a"], a["b"])
        else:
            assert getattr(ops, c.op)(a["a"], a["b"], out=a["c"]) is a["c"]
    elif c.fam == "act":
        if c.op in ("silu", "gelu", "sigmoid", "tanh", "relu2"):
            assert getattr(ops, c.op)(a["x"], out=a["y"]) is a["y"]
        else:                                   # the unary wrappers take no out=
            call("pgk_activation", a["x"]._p, a["y"]._p, c.n, R.ACT_CODES[c.op], code, None)
    elif c.fam == "glu":
        assert getattr(ops, c.op)(a["g"], a["u"], out=a["o"]) is a["o"]
    elif c.fam == "glu_packed":
        assert ops.glu_packed(a["gu"], c.shape[1], activation=c.op, out=a["o"]) is a["o"]
    elif c.fam == "bias_add":
        ops.bias_add_inplace(a["out"], a["bias"])
    elif c.fam == "cast":
        call("pgk_cast", a["src"]._p, code, a["dst"]._p, DT[c.extra[0]].code, c.n, None)
    elif c.fam == "norm":
        if c.op == "rmsnorm":
            assert ops.rmsnorm(a["x"], a["gamma"], R.EPS, out=a["out"]) is a["out"]
        elif c.op == "rmsnorm_residual":
            assert ops.rmsnorm_residual(a["x"], a["res"], a["gamma"], R.EPS, out=a["out"]) is a["out"]
        else:
            assert ops.layernorm(a["x"], a["gamma"], a["beta"], R.EPS, out=a["out"]) is a["out"]
    elif c.fam == "rope":
        (ops.rope_inplace if c.extra[0] == c.dtype else ops.rope_inplace_f32table)(a["q"], a["k"], a["cos"], a["sin"])
    elif c.fam == "reduce":
        call("pgk_reduce", a["x"]._p, a["out"]._p, c.n, R.REDUCE_CODES[c.op], code, None)
    elif c.fam == "softmax":
        call("pgk_softmax_rows", a["x"]._p, a["y"]._p, c.shape[0], c.shape[1], code, None)
    elif c.fam == "sum_axis":
        call("pgk_sum_axis", a["x"]._p, a["out"]._p, c.shape[0], c.shape[1], 0 if c.op == "axis0" else 1, code, None)
    elif c.fam == "clamp":
        call("pgk_clamp", a["x"]._p, a["y"]._p, c.n, C.c_float(R.CLAMP_LO), C.c_float(R.CLAMP_HI), code, None)
    else:
        assert c.fam == "where", c.fam
        call("pgk_where", a["cond"]._p, a["a"]._p, a["b"]._p, a["y"]._p, c.n, code, None)


def run_case(c: R.Case) -> None:
    p = place(c)
    # 1. the leaf, from the real pointers
    for name, o in p.items():
        if o.n:
            assert (o.arr.data_ptr() % 16 != 0) == (name in c.mis), f"{c}: operand {name} at {o.arr.data_ptr():#x}"
    aligned = all(o.arr.data_ptr() % 16 == 0 for o in p.values() if o.n)
    args = R.plan_args(c)
    if args is not None:
        assert ops.base_op_plan(args[0], args[1], args[2], R.DTYPE_NAME[c.dtype], aligned) == c.leaf, str(c)
    else:
        assert c.leaf is None
    twin = None
    if c.fam == "binary" and c.op.endswith("_inplace"):              # the out-of-place result of the same operands, first
        twin = getattr(ops, c.op[:-len("_inplace")])(p["a"].arr, p["b"].arr).to_numpy().view(WORD[c.dtype])
    # 2. run
    launch(c, p)
    # 3. every element of every output, 4. the guards and the inputs
    got = {}
    for name, (dt, shape, is_out) in R.operands(c).items():
        words, guards_ok = p[name].back()
        assert guards_ok, f"{c}: the padding around {name} was written"
        if is_out:
            got[name] = words
        else:
            assert (words.reshape(-1) == p[name].sent[p[name].off:p[name].off + p[name].n]).all(), f"{c}: input {name} was written"
    bad = R.mismatches(c, got)
    assert not any(m.any() for m in bad.values()), R.explain(c, got)
    if twin is not None:
        np.testing.assert_array_equal(R.canonical(got["a"], c.dtype), R.canonical(twin.reshape(got["a"].shape), c.dtype), err_msg=str(c))


@pytest.mark.parametrize("key", list(GROUPS), ids=str)
def test_every_element_on_every_branch(key):
    for c in GROUPS[key]:
        run_case(c)


def test_activation_in_place_equals_out_of_place():
    """`out` may alias the input (ops.silu docstring): same words as the out-of-place call, on both leaves."""
    for dt in R.DTYPES:
        for mis in ((), ("x",)):
            c = next(c for c in R.CASES if (c.fam, c.op, c.dtype, c.mis) == ("act", "silu", dt, mis) and c.n > 256)
            words = R.to_words(R.inputs(c)["x"], dt)
            x = Operand(words, dt, c.shape, bool(mis))
            want = ops.silu(x.arr).to_numpy().view(WORD[dt])
            ops.silu(x.arr, out=x.arr)
            got, guards_ok = x.back()
            assert guards_ok
            np.testing.assert_array_equal(got, want.reshape(got.shape))
            assert not R.mismatches(c, {"y": got})["y"].any(), R.explain(c, {"y": got})
