"""Specification of the reduced matmul precisions of the bf16x3 128x128 GEMM class ('high' and 'medium' of
twog_gemm_set_precision / HipKernels.matmul_precision / TGGCN.use_matmul_precision), as bit-level numpy functions on fp32
arrays. csrc/gemm_f32.hip (split2 / split1, gemm_mainloop_x3 with NP = 2 / 1) has to match them.

Notation. bf16 = the fp32 patterns whose low 16 bits are zero: 8 significant bits. rne(x) = x rounded to the nearest bf16, ties
to the even 8-bit significand, computed on the bit pattern: u + 0x7fff + ((u >> 16) & 1), low half cleared. For x in the
binade [2^e, 2^(e+1)) the bf16 spacing is 2^(e-7), so |x - rne(x)| <= 2^(e-8) <= 2^-8 |x|.

    round_medium(x) = rne(x)                                  'medium': one plane,  product  h_a h_b
    split_high(x)   = (h, m),  h = rne(x),  m = rne(x - h)    'high':   two planes, products h_a h_b + h_a m_b + m_a h_b

h is ROUNDED, not truncated (the choice the issue leaves open): then m = rne(x - h) takes either sign whatever the sign of x,
and the dropped product m_a m_b has no preferred sign on same-sign operands; a truncated h would make every m carry the sign
of x and m_a m_b a bias towards zero of ~2^-18 |a b|. Both products sums are accumulated in fp32 as the 'highest' kernel does.

x - h is exact in fp32: it is a multiple of ulp_fp32(x) = 2^(e-23) of magnitude <= 2^(e-8), i.e. at most 16 significant
bits. m, the 8-bit rounding of such a multiple, is a multiple of 2^(e-23) too, and |h + m| <= 2^(e+1): the sum h + m has at
most 24 significant bits and is exact in fp32 as well.

Edges.
  * Top of the exponent range: rne can reach Inf where the truncating three-way split cannot. |x| >= 0x7f7f8000 (max bf16 + half
    a spacing = 3.3961775e38; fp32 max is 3.4028235e38) gives h = +-Inf. 'medium' then multiplies by +-Inf like an overflowed
    fp32 product would; 'high' gives m = x - h = -+Inf and h + m = NaN, the same result 'highest' has for an Inf operand.
    Nothing is saturated: operands within 0.2 % of the fp32 maximum do not occur in a run that is not already broken.
  * +-Inf: h = +-Inf (the low half of the pattern is zero already). 'medium' keeps Inf arithmetic (Inf * 0 = NaN as in fp32);
    'high': m = Inf - Inf = NaN, every product that touches the operand is NaN ('highest' does the same).
  * NaN: stays NaN, quieted (bit 22 set), sign and high payload kept; m of a NaN is NaN.
  * Zeros keep their sign; m of a bf16-representable x is +0.
  * Subnormals: rounded on the bit pattern like everything else (bf16 subnormals are fp32 subnormals with a zero low half);
    the absolute error is then <= 2^-134, half the subnormal bf16 spacing, instead of 2^-8 |x|. The same holds for m whenever
    x - h is subnormal (|x| < 2^-118). (The kernel's converts and bf16 MFMA may flush subnormal planes to zero: a difference
    below 2^-126 per operand, far below anything the tests resolve.)

Per-operand bounds, U = 2^-134 the underflow term:
    |x - round_medium(x)| <= 2^-8 |x| + U                                  (E_MEDIUM = 2^-8)
    |x - h - m|           <= 2^-17 |x| + U                                 (E_HIGH   = 2^-17)
  for 'high': |x - h| <= 2^(e-8). At equality x - h is a bf16 and m is exact; below it x - h lies in a binade no higher than
  [2^(e-9), 2^(e-8)), whose bf16 spacing is 2^(e-16): |(x - h) - m| <= 2^(e-17) <= 2^-17 |x|. Also |m| <= 2^(e-8) <= 2^-8 |x|
  (2^(e-8) is a bf16: rounding cannot pass it).

Per-product constants (exact arithmetic, operands and planes in the normal range so that U plays no part).
  'medium'. a = h_a + d_a, |d_a| <= 2^-8 |a|, so |h_a| <= (1 + 2^-8) |a|; the same for b.
      a b - h_a h_b = d_a b + h_a d_b,   |.| <= (2^-8 + (1 + 2^-8) 2^-8) |a||b| = (2^-7 + 2^-16) |a||b|
      C_MEDIUM = 2^-7 + 2^-16  (<= 2^-6)
  'high'. a = h_a + m_a + e_a with |e_a| <= 2^-17 |a| and |m_a| <= 2^-8 |a|; the same for b. Write s_a = h_a + m_a = a - e_a.
      a b - (h_a h_b + h_a m_b + m_a h_b) = (a b - s_a s_b) + m_a m_b
      a b - s_a s_b = e_a b + s_a e_b,   |.| <= (2^-17 + (1 + 2^-17) 2^-17) |a||b| = (1 + 2^-18) 2^-16 |a||b|
      |m_a m_b| <= 2^-16 |a||b|
      total <= (2 + 2^-18) 2^-16 |a||b|;  C_HIGH = (2 + 2^-6) 2^-16 = 2^-14.99  (<= 2^-13), rounded up to a plain constant
  Summed over k: |sum_k kept products - sum_k a_k b_k| <= C sum_k |a_k||b_k|.
"""
import numpy as np

E_MEDIUM = 2.0 ** -8       # |x - round_medium(x)| <= E_MEDIUM |x| + U
E_HIGH = 2.0 ** -17        # |x - h - m|           <= E_HIGH |x| + U
U = 2.0 ** -134            # underflow term: half the spacing of the bf16 subnormals
C_MEDIUM = 2.0 ** -7 + 2.0 ** -16
C_HIGH = (2.0 + 2.0 ** -6) * 2.0 ** -16


def _rne_bits(u):
    """uint32 patterns -> the patterns of their nearest bf16 (ties to even), as uint32 with a zero low half."""
    u = u.astype(np.uint32)
    r = ((u.astype(np.uint64) + 0x7fff + ((u >> 16) & 1)) & 0xffff0000).astype(np.uint32)   # (64-bit: no wrap at 0xffff....)
    nan = (u & 0x7fffffff) > 0x7f800000
    return np.where(nan, (u & 0xffff0000) | 0x00400000, r).astype(np.uint32)


def round_medium(x):
    """fp32 array -> its round-to-nearest-even bf16 plane (fp32 values whose low 16 pattern bits are zero)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    return _rne_bits(x.view(np.uint32)).view(np.float32).reshape(x.shape)


def split_high(x):
    """fp32 array -> (h, m): h = rne(x), m = rne(x - h), both bf16-representable fp32 arrays."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    h = round_medium(x)
    with np.errstate(invalid='ignore'):
        m = round_medium(x - h)   # exact subtraction (module docstring)
    return h, m


def kept_products(a, b, mode):
    """The sum over k of the kept chunk products of a (M, K) and b (K, N) in fp64 -- what the kernel would give with an
    exact accumulator. mode: 'high' or 'medium'."""
    if mode == 'medium':
        return round_medium(a).astype(np.float64) @ round_medium(b).astype(np.float64)
    assert mode == 'high', mode
    (ha, ma), (hb, mb) = split_high(a), split_high(b)
    ha, ma, hb, mb = (v.astype(np.float64) for v in (ha, ma, hb, mb))
    return ha @ hb + ha @ mb + ma @ hb
