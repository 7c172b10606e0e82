"""Device-memory plumbing for the GPU parity tests (torch = allocator only)."""
import numpy as np


# torch fills / copies on its own stream; the library works on another one, so
# every helper waits for torch before handing the buffer over (without this a
# late zero-fill can overwrite what the library already wrote)
def to_dev(arr: np.ndarray):
    import torch
    a = np.ascontiguousarray(arr).view(np.int64)
    t = torch.from_numpy(a.copy()).to("cuda")
    torch.cuda.synchronize()
    return t


def from_dev(t, shape_last=4) -> np.ndarray:
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64).reshape(-1, shape_last)


def empty_dev(n_elems: int, limbs: int = 4):
    import torch
    t = torch.zeros((n_elems, limbs), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    return t


def proof_after_tables(ctx, prove, names):
    """(proof, counters) of the proof that follows the context's table build:
    a proof that finds the optional tables missing goes without them and has
    them built in the background (context.h, "Deferred tables"); ctx.sync()
    waits for that build, and the next proof, made with kernel timing on, uses
    them.  prove(ctx) returns a ProofC; both proofs must be the same bytes."""
    from pnp import abi
    first = prove(ctx)
    ctx.sync()
    ctx.kernel_timing(True)
    got = prove(ctx)
    assert abi.proof_to_bytes(got) == abi.proof_to_bytes(first)
    return got, {k: ctx.kernel_bytes(k) for k in names}


def second_proof_counters(load, prove, names, after=None):
    """proof_after_tables on a fresh context that load(ctx) gives its keys;
    after(ctx, proof) runs before the context is closed."""
    import pnp
    ctx = pnp.Context(0)
    try:
        load(ctx)
        got, c = proof_after_tables(ctx, prove, names)
        if after is not None:
            after(ctx, got)
        return got, c
    finally:
        ctx.close()


def host_keys(inp):
    """load(ctx) for second_proof_counters: the instance's keys from host pointers."""
    def load(ctx):
        ctx.load_prover_key(inp.pk, inp.n, device_ptrs=False)
        ctx.load_commit_key(inp.ck, inp.n, device_ptrs=False)
    return load
