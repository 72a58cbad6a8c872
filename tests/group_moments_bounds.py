"""DERIVED per-element bounds of mmvae_gemm_nt_group_moments (csrc/group_moments.hip) against its float64 restatement
(tests/group_moments_ref.py), in the manner of tests/gemm_bounds.py, whose rules for the product and the sigmoid they continue.  The
model of one float32 operation and every constant are those of tests/elementwise_bounds.py (U = 2^-24 one rounding, ULP = 2 U one
hardware ulp, E_SQRT the hardware root, SECOND the second-order terms); nothing below was fitted to what a kernel returns.

  x_g        = act(sum_k a w + bias): gemm_bounds.nt_tol, then gemm_bounds.sigmoid_tol where the activation is the sigmoid   (tol_x)
  mean       m = (sum_g x_g) / G.  Every term enters with its own tol_x; G fp32 terms summed in ANY order, (G - 1) U sum_g |x_g|;
             one division (a scaling: one rounding), U |sum| / G:
                 tol_m = SECOND (sum_g tol_x / G + G U sum_g (|x_g| + tol_x) / G)
  deviation  d_g = x_g - m, both as the kernel has them: tol_x + tol_m, plus one rounding of the difference:
                 tol_d = SECOND (tol_x + tol_m + U |d_g|)
  squares    ss = sum_g d_g^2.  A square of a value within tol_d of d: first order 2 |d| tol_d, second order tol_d^2.  G terms, each
             product and each addition (or their fused form) rounded: at most G U on the sum of the squares as the kernel has them:
                 tol_ss = SECOND (sum_g (2 |d_g| tol_d + tol_d^2) + G U sum_g (|d_g| + tol_d)^2)
  variance   v = ss / (G - 1), one rounding:   tol_v = SECOND (tol_ss + U (ss + tol_ss)) / (G - 1)
  std        the root is monotone: the kernel's std lies in [sqrt(max(v - tol_v, 0)), sqrt(v + tol_v)], plus one ulp of the hardware
             root (E_SQRT) of the upper end:   tol_s = max(hi - s, s - lo) + E_SQRT hi
Where the members of a group are identical the exact spread is 0 and the bound is sqrt(tol_v): the root's own sensitivity at 0.
"""
import numpy as np

import gemm_bounds as GB
from elementwise_bounds import U, E_SQRT, SECOND

ACT_SIGMOID = 2
_f = GB._f


def x_ref_tol(a, w, bias, act):
    """-> (x float64 [M][N], tol_x)"""
    v, tol = GB.nt_ref(a, w, bias), GB.nt_tol(a, w, bias)
    if act == ACT_SIGMOID:
        return GB.sigmoid(v), GB.sigmoid_tol(v, tol)
    return v, tol


def moments_tol(x, tol_x, G):
    """x, tol_x [B G][N] -> (mean, tol_mean, std, tol_std) [B][N]; std and tol_std None for G == 1"""
    x, tol_x = _f(x), np.broadcast_to(_f(tol_x), np.shape(x))
    N = x.shape[1]
    x, tol_x = x.reshape(-1, G, N), tol_x.reshape(-1, G, N)
    m = x.mean(1)
    tol_m = SECOND * (tol_x.sum(1) / G + G * U * (np.abs(x) + tol_x).sum(1) / G)
    if G == 1:
        return m, tol_m, None, None
    d = x - m[:, None, :]
    tol_d = SECOND * (tol_x + tol_m[:, None, :] + U * np.abs(d))
    ss = (d * d).sum(1)
    tol_ss = SECOND * ((2 * np.abs(d) * tol_d + tol_d ** 2).sum(1) + G * U * ((np.abs(d) + tol_d) ** 2).sum(1))
    v = ss / (G - 1)
    tol_v = SECOND * (tol_ss + U * (ss + tol_ss)) / (G - 1)
    s, hi, lo = np.sqrt(v), np.sqrt(v + tol_v), np.sqrt(np.maximum(v - tol_v, 0.0))
    return m, tol_m, s, np.maximum(hi - s, s - lo) + E_SQRT * hi


def problem_tol(a, w, bias, act, G):
    """The whole entry point from its (bf16-valued) operands -> (mean, tol_mean, std, tol_std)"""
    x, tol_x = x_ref_tol(a, w, bias, act)
    return moments_tol(x, tol_x, G)
