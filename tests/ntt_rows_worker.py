"""Child process of tests/test_gpu_blocks.py::test_plain_twiddle_table: the
switch PNP_NTT_ROWS is read once per process, so the transforms that read the
plain twiddle table run here.  Prints one line per check and ROWS_OFF_OK."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(os.path.dirname(HERE), "zprize23-gpu-submission_amd")]


def main():
    assert os.environ.get("PNP_NTT_ROWS") == "0"
    import pnp
    from block_gpu import check_lde_intt, check_ntt
    from pnp_testlib import rand_fr_mont_arr
    ctx = pnp.Context(0)
    try:
        for lg in (11, 12):  # two passes: (6, 5) and (6, 6)
            check_ntt(ctx, rand_fr_mont_arr(np.random.default_rng(300 + lg), 1 << lg), lg)
            print("ntt", lg)
        # one pass K = 7, 8, 9, 10; two passes (6, 5) and (6, 6): every K of 5..10,
        # DIF with the fused twist and DIT with the fused post-twist
        for lg, m0, nb in [(7, 0, 8), (8, 0, 8), (9, 0, 8), (9, 0, 6), (10, 0, 7), (11, 0, 6), (12, 0, 8),
                           (12, 0, 7)]:
            check_lde_intt(ctx, lg, m0, nb)
            print("blocks", lg, m0, nb)
    finally:
        ctx.close()
    print("ROWS_OFF_OK")


if __name__ == "__main__":
    main()
