"""geobo_transpose (the lower-left block of AkA from the computed upper-right one) against torch: exact, ragged against the 64 x 64
tile, more than one tile both ways, inside a larger buffer whose other entries keep their bits."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("rows,cols", [(1, 1), (64, 64), (65, 130), (200, 70)])
def test_transpose_is_exact_and_stays_inside(rows, cols):
    from geobo_amd import hip
    hip.require_gpu()
    g = torch.Generator(device="cpu").manual_seed(rows + cols)
    big = torch.rand((rows + cols + 3, rows + cols + 5), generator=g, dtype=torch.float64).cuda()
    before = big.clone()
    src = big[:rows, rows + 2:rows + 2 + cols]                    # upper-right block
    dst = big[rows + 1:rows + 1 + cols, 1:1 + rows]               # lower-left block
    hip.transpose(src, dst)
    assert bool((dst == before[:rows, rows + 2:rows + 2 + cols].t()).all())
    big[rows + 1:rows + 1 + cols, 1:1 + rows] = before[rows + 1:rows + 1 + cols, 1:1 + rows]
    assert bool((big.view(torch.int64) == before.view(torch.int64)).all())
