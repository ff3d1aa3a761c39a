"""CPU: the vectorised unpacking of the update kernels' packed bfloat16 images (tests/update_check_util.py) is the loop of mlp.unpack_rows."""
import torch

from update_check_util import unpack_rows


def test_fast_unpack_equals_the_loop():
    from gym_continuousdoubleauction_amd import mlp
    g = torch.Generator().manual_seed(1)
    for n_rows, n_feat, paired in ((64, 192, False), (96, 512, True), (32, 32, False), (64, 224, False)):
        packed = torch.randn(n_rows * n_feat, generator=g).to(torch.bfloat16)
        want = mlp.unpack_rows(packed, n_rows, n_feat, paired=paired)
        assert torch.equal(unpack_rows(packed, n_rows, n_feat, paired=paired), want)
        # a row range of the image (multiples of 32 rows)
        assert torch.equal(unpack_rows(packed, n_rows - 32, n_feat, paired=paired, first_row=32), want[32:])
