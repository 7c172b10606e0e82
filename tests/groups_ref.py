"""A CPU model of the copy-group builder (csrc/wires.hip), in plain Python
integers over the four sigma columns of a circuit.

It restates what the builder documents, not how it computes it:

  * sigma_j(w^i) = k_j' w^i' (K = 1, 7, 13, 17) gives every position
    p = j n + i its successor j' n + i'; the orbits are the cycles;
  * wire j's groups are the cycles restricted to wire j, ordered by the
    smallest position of the WHOLE cycle, rows in row order inside a group;
    laid end to end in that order, a group covers sorted positions [t0, t1)
    and is summed in pieces of 32: (t1 - 1) // 32 - t0 // 32 + 1 of them;
  * z's runs: a run starts at row 0 and after every row sigma does not fix in
    all four wires (z_(i+1) = z_i there and only there);
  * a group or run of more than 256 pieces is heavy (a workgroup of its own);
  * a wire is ident (its scalars are its evaluations) when 10 g > 9 n; the
    wires are committed over their groups when some wire that is not ident has
    4 g < 3 n; z is when not 10 g_z > 9 n;
  * per proof, the groups are used only when every group of a wire that is not
    ident holds one value.

Segments are indexed 0..3 = wires a..d, 4 = z."""
from pnp_testlib import R_MOD, fr_root, fr_unmont, from_limbs, oracle, vp

K = (1, 7, 13, 17)
PIECE = 32    # positions a piece covers
HEAVY = 256   # more pieces than this: heavy
SIGMA = ("left_sigma", "right_sigma", "out_sigma", "fourth_sigma")


def pieces(t0: int, t1: int) -> int:
    return (t1 - 1) // PIECE - t0 // PIECE + 1


def sigma_of(inp):
    """The four sigma columns (canonical ints) of a GeneralInputs or Inputs:
    the forward transform of the key's coefficients."""
    cols = []
    for name in SIGMA:
        c = inp.arrays[name + "_coeffs"].copy()
        oracle().or_ntt(vp(c), inp.lg_n, 0, 0)
        cols.append([fr_unmont(from_limbs(r)) for r in c])
    return cols


class GroupModel:
    def __init__(self, sig, n: int):
        assert n & (n - 1) == 0 and all(len(c) == n for c in sig)
        self.n = n
        w = fr_root(n.bit_length() - 1)
        where = {}
        x = 1
        for i in range(n):
            for j in range(4):
                where[K[j] * x % R_MOD] = j * n + i
            x = x * w % R_MOD
        assert len(where) == 4 * n
        # the successor of every position, and the cycles
        self.next = [where[sig[p // n][p % n]] for p in range(4 * n)]
        assert sorted(self.next) == list(range(4 * n)), "sigma is no permutation of the 4n positions"
        label = [None] * (4 * n)
        self.cycles = []
        for p in range(4 * n):  # ascending: p is the smallest position of a cycle not yet seen
            if label[p] is not None:
                continue
            cyc, q = [], p
            while label[q] is None:
                label[q] = p
                cyc.append(q)
                q = self.next[q]
            self.cycles.append(cyc)
        self.label = label
        # per wire: groups in label order, rows in row order
        self.groups = []
        for j in range(4):
            by = {}
            for i in range(n):
                by.setdefault(label[j * n + i], []).append(i)
            self.groups.append([by[k] for k in sorted(by)])
        # z: runs of rows, in row order
        heads = [i for i in range(n)
                 if i == 0 or any(self.next[j * n + i - 1] != j * n + i - 1 for j in range(4))]
        self.groups.append([list(range(a, b)) for a, b in zip(heads, heads[1:] + [n])])
        self.g = [len(gr) for gr in self.groups]
        self.runs, self.pieces, self.heavy = [], [], []
        for gr in self.groups:
            t, runs = 0, []
            for rows in gr:
                runs.append((t, t + len(rows)))
                t += len(rows)
            assert t == n
            self.runs.append(runs)
            self.pieces.append([pieces(a, b) for a, b in runs])
            self.heavy.append(sum(1 for k in self.pieces[-1] if k > HEAVY))
        # the decisions, with the builder's integer comparisons
        self.ident = [10 * g > 9 * n for g in self.g]
        self.wires_ok = any(not self.ident[j] and 4 * self.g[j] < 3 * n for j in range(4))
        self.z_ok = not self.ident[4]
        # a segment is summed (and its heavy groups queued) only when it is not ident
        self.heavy_queued = [0 if self.ident[s] else self.heavy[s] for s in range(5)]

    def one_value(self, col, j: int) -> bool:
        """Does every group of wire j hold one value in col (n values, padded)?"""
        return all(len({col[i] for i in rows}) == 1 for rows in self.groups[j])

    def witness_keeps_groups(self, cols) -> bool:
        """What the per-proof check decides: the wires that are not ident."""
        return all(self.ident[j] or self.one_value(cols[j], j) for j in range(4))

    def counters(self, cols=None) -> dict:
        """The counters of a timed proof on a context whose groups are built
        (cols: the four padded witness columns; None: a witness that keeps
        its copy constraints)."""
        keeps = cols is None or self.witness_keeps_groups(cols)
        c = {"wire_groups_used": int(self.wires_ok and keeps),
             "wire_group_fallback": int(self.wires_ok and not keeps),
             "z_groups_used": int(self.z_ok), "z_group_fallback": 0}
        for s, name in enumerate("abcdz"):
            c["groups_found_" + name] = self.g[s]
            c["groups_heavy_" + name] = self.heavy_queued[s]
        return c


COUNTERS = ("wire_groups_used", "wire_group_fallback", "z_groups_used", "z_group_fallback") + tuple(
    "groups_%s_%s" % (k, s) for s in "abcdz" for k in ("found", "heavy"))


def witness_columns(inp):
    """The four padded witness columns of an instance (Montgomery ints: only
    equality matters)."""
    cols = []
    for name in ("w_l", "w_r", "w_o", "w_4"):
        col = [from_limbs(r) for r in inp.arrays[name]]
        cols.append(col + [0] * (inp.n - len(col)))
    return cols


def model_of(inp) -> GroupModel:
    return GroupModel(sigma_of(inp), inp.n)
