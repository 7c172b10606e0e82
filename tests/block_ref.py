"""Reference of round 4's block-layout transforms (csrc/ntt.hip lde_blocks,
to_blocks, intt_blocks, t_combine_blocks, t_combine), from the oracle's
transforms and Python integers only.

n = 2^lg.  The 8n coset x_i = g w_8n^i (g = 7) is kept in block-bitrev layout:
point i = 8 j + m lives in block m at index brev(j), brev the lg-bit reversal.

Two layers.  The *_ints functions are the defining formulas on lists of
integers mod r, as O(n^2) sums; every formula is linear in its input, so they
hold for canonical values and for Montgomery representatives alike.  The
ref_* functions are what the GPU tests compare with, on (count, 4) uint64
Montgomery limb arrays, and lean on or_coset_lde8 / or_ntt for the size-n
transforms; tests/test_block_ref.py holds them to the formulas.
"""
import numpy as np

from pnp_testlib import R_MOD, FR_GEN, fr_root, oracle, vp

_MASK = (1 << 64) - 1


# ------------------------------------------------------------------ limbs <-> integers
def to_obj(arr: np.ndarray) -> np.ndarray:
    """(count, 4) uint64 limbs -> object array of Python integers."""
    a = np.asarray(arr, dtype=np.uint64).reshape(-1, 4).astype(object)
    return a[:, 0] + (a[:, 1] << 64) + (a[:, 2] << 128) + (a[:, 3] << 192)


def from_obj(v) -> np.ndarray:
    v = np.asarray(v, dtype=object)
    out = np.empty((len(v), 4), dtype=np.uint64)
    for k in range(4):
        out[:, k] = ((v >> (64 * k)) & _MASK).astype(np.uint64)
    return out


def brev_index(lg: int) -> np.ndarray:
    """brev_index(lg)[j] = the lg-bit reversal of j."""
    idx = np.arange(1 << lg, dtype=np.int64)
    r = np.zeros_like(idx)
    for k in range(lg):
        r |= ((idx >> k) & 1) << (lg - 1 - k)
    return r


def _powers(base: int, count: int) -> np.ndarray:
    out = np.empty(count, dtype=object)
    p = 1
    for i in range(count):
        out[i] = p
        p = p * base % R_MOD
    return out


# ------------------------------------------------------------------ the formulas, O(n^2)
def coset_evals_ints(c, lg: int):
    """E[i] = sum_k c_k (g w_8n^i)^k, i < 8n (Horner, any number of coefficients)."""
    w = fr_root(lg + 3)
    out, x = [], FR_GEN
    for _ in range(8 << lg):
        acc = 0
        for ck in reversed(c):
            acc = (acc * x + ck) % R_MOD
        out.append(acc)
        x = x * w % R_MOD
    return out


def intt_block_ints(blk, lg: int, m: int):
    """Y_m[u] = w_8n^(-m u) sum_j blk[j] w_n^(-j u), blk in natural order, no 1 / n."""
    n = 1 << lg
    wn_inv = pow(fr_root(lg), -1, R_MOD)
    w8n_inv = pow(fr_root(lg + 3), -1, R_MOD)
    wp = [pow(wn_inv, e, R_MOD) for e in range(n)]
    return [pow(w8n_inv, m * u, R_MOD) * sum(blk[j] * wp[j * u % n] for j in range(n)) % R_MOD
            for u in range(n)]


def combine_ints(Y, lg: int, nb: int, q0: int = 0):
    """Y: the 8 lists Y_m[u], u in [q0, q0 + len).  Returns (out, nz):
    out[m1 len + (u - q0)] = c_(u + n m1) = g^-(u + n m1) / (8n) sum_m w_8^(-m m1) Y_m[u]
    for the chunks m1 < nb, and nz with bit m1 set iff chunk m1 is not all zero."""
    n = 1 << lg
    length = len(Y[0])
    w8_inv = pow(fr_root(3), -1, R_MOD)
    g_inv = pow(FR_GEN, -1, R_MOD)
    inv8n = pow(8 * n, -1, R_MOD)
    out, nz = [], 0
    for m1 in range(nb):
        for k in range(length):
            s = sum(Y[m][k] * pow(w8_inv, m * m1 % 8, R_MOD) for m in range(8))
            v = s * pow(g_inv, q0 + k + n * m1, R_MOD) % R_MOD * inv8n % R_MOD
            out.append(v)
            if v:
                nz |= 1 << m1
    return out, nz


# ------------------------------------------------------------------ on limb arrays
def coset_lde8(coeffs: np.ndarray, lg: int) -> np.ndarray:
    """or_coset_lde8: the 8n coset values of the n coefficients, natural order."""
    E = np.zeros((8 << lg, 4), dtype=np.uint64)
    oracle().or_coset_lde8(vp(np.ascontiguousarray(coeffs)), vp(E), lg)
    return E


def ref_to_blocks(a8: np.ndarray, lg: int, m0: int, nb: int) -> np.ndarray:
    """out[b n + brev(j)] = a8[8 j + m0 + b], b < nb."""
    n = 1 << lg
    v = np.asarray(a8, dtype=np.uint64).reshape(n, 8, 4)
    p = brev_index(lg)
    out = np.empty((nb, n, 4), dtype=np.uint64)
    for b in range(nb):
        out[b, p] = v[:, m0 + b]
    return out.reshape(nb * n, 4)


def ref_lde_blocks(coeffs: np.ndarray, lg: int, m0: int, nb: int, form29: bool = False, E=None) -> np.ndarray:
    """out[b n + brev(j)] = E[8 j + m0 + b], E = or_coset_lde8(coeffs) (or the
    one handed in); form29: 32 E mod r, canonical."""
    if E is None:
        E = coset_lde8(coeffs, lg)
    out = ref_to_blocks(E, lg, m0, nb)
    if form29:
        out = from_obj(to_obj(out) * 32 % R_MOD)
    return out


def ref_intt_blocks(blocks: np.ndarray, lg: int, m0: int, nb: int) -> np.ndarray:
    """Block b (residue m = m0 + b, block-bitrev layout) -> Y_m, natural order:
    n or_ntt(inverse) of the natural-order block, times w_8n^(-m u), in integers."""
    n = 1 << lg
    p = brev_index(lg)
    w8n_inv = pow(fr_root(lg + 3), -1, R_MOD)
    out = np.empty((nb * n, 4), dtype=np.uint64)
    for b in range(nb):
        nat = np.ascontiguousarray(blocks[b * n:(b + 1) * n][p])  # nat[j] = blk[brev(j)]
        oracle().or_ntt(vp(nat), lg, 1, 0)
        tw = _powers(pow(w8n_inv, m0 + b, R_MOD), n)
        out[b * n:(b + 1) * n] = from_obj(to_obj(nat) * (tw * n % R_MOD) % R_MOD)
    return out


def ref_t_combine(Y8: np.ndarray, lg: int, nb: int, q0: int = 0, length=None):
    """Y8: all 8 blocks Y_m (8 n, natural order).  The formula of combine_ints
    on u in [q0, q0 + length), vectorised: (out (nb length, 4), nz)."""
    n = 1 << lg
    if length is None:
        length = n - q0
    w8_inv = pow(fr_root(3), -1, R_MOD)
    g_inv = pow(FR_GEN, -1, R_MOD)
    inv8n = pow(8 * n, -1, R_MOD)
    Y = [to_obj(Y8[m * n + q0:m * n + q0 + length]) for m in range(8)]
    gu = _powers(g_inv, q0 + length)[q0:]
    out = np.empty((nb * length, 4), dtype=np.uint64)
    nz = 0
    for m1 in range(nb):
        s = sum(Y[m] * pow(w8_inv, m * m1 % 8, R_MOD) for m in range(8)) % R_MOD
        c = s * (gu * (pow(g_inv, n * m1, R_MOD) * inv8n % R_MOD) % R_MOD) % R_MOD
        out[m1 * length:(m1 + 1) * length] = from_obj(c)
        if any(int(v) != 0 for v in c):
            nz |= 1 << m1
    return out, nz
