"""The block counts of the shared column reducer's plan (csrc/kernels/col_reduce.h) that are reachable without a GPU:
``bn_bwd_reduce_blocks`` and ``bn_bwd_reduce32_blocks`` are host-only bindings.  A block is 256 // groups row lanes
(groups = C / 8 for 16-bit, C / 4 for fp32, one row lane from 256 groups on); both rules ask for at least 16 rows per
thread and stop at 1024 blocks.  The counts are part of the result bits, so an edit of the plan must not move them."""
import pytest

WIDTHS = [8, 24, 64, 192, 1280, 2048]
ROWS = [1, 15, 4096, 4097, 40009, 1200 * 56 * 56]


def _blocks(rows, groups):
    rpi = 256 // min(groups, 256)
    return max(1, min(1024, -(-rows // (rpi * 16))))


@pytest.mark.parametrize("C", WIDTHS)
def test_bn_bwd_reduce_block_counts(C):
    from pytorch_distributed_template_amd.ops import native
    for rows in ROWS:
        assert native.C.bn_bwd_reduce_blocks(rows, C) == _blocks(rows, C // 8), (rows, C)
        assert native.C.bn_bwd_reduce32_blocks(rows, C) == _blocks(rows, C // 4), (rows, C)
