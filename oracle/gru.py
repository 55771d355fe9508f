"""Plain-torch restatement of the whole-sequence GRU kernels (focal_gru_seq_fwd / _bwd), in the kernels' own layout
(test infrastructure; see oracle/__init__.py and oracle/deepsense.py::gru_direction).

One direction of one nn.GRU layer with h0 = 0, gate order (r, z, n):
    n = tanh(gi_n + r * (W_hn h + b_hn)),   h' = (1 - z) n + z h.
The input projections gi (incl. b_ih) are an argument: the kernels get them from a GEMM in front.

The kernels make ONE deliberate approximation: W_hh is stored in bf16 and the operand of each recurrent product (h forward,
dgh backward) is rounded to bf16 for the matrix cores; accumulation and every gate formula are fp32.  `round_operand` states
that rounding; with it off (and `round_weight` as needed) the functions are nn.GRU in `dtype`, which
tests/test_gru_reference_cpu.py shows against torch.nn.GRU and autograd before the reference judges a kernel.
"""
import torch


def bf16_round(x):
    """x rounded to the nearest bf16 value, in x's own dtype."""
    return x.to(torch.bfloat16).to(x.dtype)


def _weight(w_hh, dtype, round_weight):
    w = w_hh.detach().to("cpu")
    return (w.to(torch.bfloat16) if round_weight else w).to(dtype)


def gru_seq_reference(gi, w_hh, b_hh, T, reverse, dtype=torch.float64, round_operand=True, round_weight=True):
    """gi [B*T, 3H] or [B, T, 3H] (rows (b, t)), w_hh [3H, H], b_hh [3H] -> (out [B, T, H], hs [T+1, B, H], save [T, 4, B, H]).
    Step s works on time t = s (forward) or T-1-s (reverse); hs[0] = 0, hs[s+1] is the state after step s;
    save[s] = r, z, n, W_hn h + b_hn of step s."""
    H = w_hh.shape[1]
    gi = gi.detach().to("cpu").to(dtype).reshape(-1, T, 3 * H)
    B = gi.shape[0]
    w = _weight(w_hh, dtype, round_weight)
    b = b_hh.detach().to("cpu").to(dtype)
    out = torch.zeros(B, T, H, dtype=dtype)
    hs = torch.zeros(T + 1, B, H, dtype=dtype)
    save = torch.zeros(T, 4, B, H, dtype=dtype)
    for s in range(T):
        t = T - 1 - s if reverse else s
        h = hs[s]
        gh = (bf16_round(h) if round_operand else h) @ w.t() + b
        r = torch.sigmoid(gi[:, t, :H] + gh[:, :H])
        z = torch.sigmoid(gi[:, t, H:2 * H] + gh[:, H:2 * H])
        ghn = gh[:, 2 * H:]
        n = torch.tanh(gi[:, t, 2 * H:] + r * ghn)
        h_new = (1 - z) * n + z * h
        hs[s + 1] = h_new
        out[:, t] = h_new
        save[s, 0], save[s, 1], save[s, 2], save[s, 3] = r, z, n, ghn
    return out, hs, save


def gru_seq_backward_reference(dout_dir, scale, w_hh, hs, save, T, reverse, dtype=torch.float64, round_operand=True,
                               round_weight=True):
    """dout_dir [B, T, H]: the upstream gradient of this direction's half of the layer output (a [B, H] gradient through a
    mean over time is that tensor broadcast over t, with scale = 1/T).  hs / save as returned by gru_seq_reference.
    -> (dgi [B, T, 3H], dgh [T, B, 3H]): the gradients of the step's input projections and of its recurrent product
    W_hh h + b_hh (dgh[s] belongs to step s, not to time t)."""
    H = w_hh.shape[1]
    dout = dout_dir.detach().to("cpu").to(dtype)
    B = dout.shape[0]
    w = _weight(w_hh, dtype, round_weight)
    hs = hs.detach().to("cpu").to(dtype)
    save = save.detach().to("cpu").to(dtype)
    dgi = torch.zeros(B, T, 3 * H, dtype=dtype)
    dgh = torch.zeros(T, B, 3 * H, dtype=dtype)
    dhrec = torch.zeros(B, H, dtype=dtype)
    dhz = torch.zeros(B, H, dtype=dtype)
    for s in range(T - 1, -1, -1):
        t = T - 1 - s if reverse else s
        r, z, n, ghn = save[s]
        h_prev = hs[s]
        dh = scale * dout[:, t] + dhrec + dhz
        dn = dh * (1 - z) * (1 - n * n)
        dz = dh * (h_prev - n) * z * (1 - z)
        dr = dn * ghn * r * (1 - r)
        dgi[:, t] = torch.cat([dr, dz, dn], 1)
        dgh[s] = torch.cat([dr, dz, dn * r], 1)
        dhz = dh * z
        dhrec = (bf16_round(dgh[s]) if round_operand else dgh[s]) @ w
    return dgi, dgh
