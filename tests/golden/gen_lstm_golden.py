"""Records tests/golden/g9_lstm.npz from torch.nn.LSTM in float64 on the CPU (the authority for the "PyTorch-compatible"
LSTM ops; the reference has no CPU path for them).  Only this generator imports torch: the tests read the fixture.

    python tests/golden/gen_lstm_golden.py

Two cases with inputs and outputs: unidirectional (B,S,I,H) = (2,5,24,20) with h0 / c0, forwards and reversed (keys u_*),
and bidirectional (2,6,16,8) from zero state (keys b_*).  Inputs come from tests/lstm_ref.py's make_case."""

from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
from tests.lstm_ref import WEIGHTS, make_bidir_case, make_case  # noqa: E402

UNI, UNI_SEED = (2, 5, 24, 20), 901
BI, BI_SEED = (2, 6, 16, 8), 902


def _set(lstm: torch.nn.LSTM, d: dict, src_sfx: str, dst_sfx: str) -> None:
    with torch.no_grad():
        for k, name in zip(WEIGHTS, ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")):
            getattr(lstm, name + dst_sfx).copy_(torch.from_numpy(d[k + src_sfx]))


def main() -> None:
    rec = {}
    B, S, I, H = UNI
    d = make_case(B, S, I, H, UNI_SEED)
    lstm = torch.nn.LSTM(I, H, batch_first=True).double()
    _set(lstm, d, "", "")
    x, h0, c0 = (torch.from_numpy(d[k]) for k in ("x", "h0", "c0"))
    with torch.no_grad():
        out, (hn, cn) = lstm(x, (h0[None], c0[None]))
        # reversed: the same layer over the time-flipped sequence, output flipped back
        outr, (hnr, cnr) = lstm(torch.flip(x, [1]), (h0[None], c0[None]))
    rec.update({f"u_{k}": v for k, v in d.items()})
    rec.update(u_out=out.numpy(), u_hn=hn[0].numpy(), u_cn=cn[0].numpy(), u_out_rev=torch.flip(outr, [1]).numpy(),
               u_hn_rev=hnr[0].numpy(), u_cn_rev=cnr[0].numpy())

    B, S, I, H = BI
    d = make_bidir_case(B, S, I, H, BI_SEED)
    lstm = torch.nn.LSTM(I, H, batch_first=True, bidirectional=True).double()
    _set(lstm, d, "_fwd", "")
    _set(lstm, d, "_bwd", "_reverse")
    with torch.no_grad():
        out, (hn, cn) = lstm(torch.from_numpy(d["x"]))
    rec.update({f"b_{k}": v for k, v in d.items()})
    rec.update(b_out=out.numpy(), b_hn=hn.numpy(), b_cn=cn.numpy())
    np.savez(os.path.join(HERE, "g9_lstm.npz"), **rec)
    print({k: v.shape for k, v in rec.items()})


if __name__ == "__main__":
    main()
