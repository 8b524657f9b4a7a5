"""A coarse entry of csrc/blocks.hip on a workspace of exactly its *_ws_bytes: shared by tests/test_gpu_e2e.py (production shapes) and
tests/test_gpu_blocks.py (the dispatch edges)."""
import torch

GUARD = 4096


def check_exact_workspace(need, call, reset, outputs, want):
    """A coarse entry of csrc/blocks.hip on a workspace of exactly its *_ws_bytes.  call(ws, ws_bytes) -> status runs the entry through the C ABI;
    reset() puts back what it updates in place or writes; outputs() are those tensors, want what the Python wrapper computed with a workspace of its
    own.  The workspace sits between two guards inside a buffer filled with 0xA5: the call leaves both guards alone and gives the wrapper's bits;
    with one byte less it answers PSAM_EWORKSPACE and touches nothing."""
    assert need > 0 and need % 256 == 0
    buf = torch.full((GUARD + need + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    reset()
    assert call(buf.data_ptr() + GUARD, need) == 0
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + need:] == 0xA5).all()), "the call wrote outside its workspace"
    assert len(outputs()) == len(want) and all(torch.equal(a, b) for a, b in zip(outputs(), want))
    reset()
    before = [t.clone() for t in outputs()]
    assert call(buf.data_ptr() + GUARD, need - 1) == -3      # PSAM_EWORKSPACE
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outputs(), before))
