"""Which tensors reach the "8 channels per thread" kernels, as a table:
ops/_vec8.py vec8_supported over channel width, rank, dtype and device.
The predicate is host code, so this runs without a GPU."""

import itertools

import pytest
import torch

from bdbnn_amd.ops import _vec8, activations, bn_act, pool
from bdbnn_amd.ops._vec8 import tensor_vec8_supported, vec8_supported

WIDTHS = [1, 2, 4, 8, 48, 64, 1024, 2048]
DIMS = [2, 4]
DTYPES = [torch.float16, torch.bfloat16, torch.float32, torch.float64]

# written out, not computed: the widths chan_map8 can index
GOOD_WIDTHS = {8, 64, 1024}
GOOD_DTYPES = {torch.bfloat16, torch.float32}

TABLE = list(itertools.product([False, True], DIMS, WIDTHS, DTYPES))


def _id(row):
    cuda, dim, C, dtype = row
    return (f"{'cuda' if cuda else 'cpu'}-{dim}d-C{C}-"
            f"{str(dtype).split('.')[-1]}")


@pytest.mark.parametrize("row", TABLE, ids=[_id(r) for r in TABLE])
def test_vec8_supported_table(row):
    cuda, dim, C, dtype = row
    want = cuda and dim == 4 and C in GOOD_WIDTHS and dtype in GOOD_DTYPES
    assert vec8_supported(cuda, dim, C, dtype) is want


def test_table_has_both_answers():
    got = [vec8_supported(*r) for r in TABLE]
    assert sum(got) == len(GOOD_WIDTHS) * len(GOOD_DTYPES)
    assert len(TABLE) == 2 * 2 * 8 * 4


@pytest.mark.parametrize("C", list(range(0, 20)) + [24, 96, 512, 1023, 1025,
                                                    4096])
def test_width_rule(C):
    want = C in (8, 16, 32, 64, 128, 256, 512, 1024)
    assert vec8_supported(True, 4, C, torch.float32) is want


class _NoSize:
    """A 2-D stand-in whose size() must not be asked for a channel."""
    is_cuda = True
    dtype = torch.float32

    def dim(self):
        return 2

    def size(self, i):
        raise AssertionError("size() indexed before dim was known")


def test_tensor_predicate_does_not_index_before_dim():
    assert tensor_vec8_supported(_NoSize()) is False
    for shape in [(), (5,), (3, 8), (2, 8, 4), (2, 8, 4, 4, 4)]:
        assert tensor_vec8_supported(torch.zeros(shape)) is False


def test_cpu_tensors_take_the_torch_path():
    """4-channel, fp16 and fp64 CPU tensors through the three modules: the
    composition, whatever the native extension would have accepted."""
    torch.manual_seed(0)
    for C, dtype in [(4, torch.float32), (8, torch.float64),
                     (8, torch.float32)]:
        x = torch.randn(2, C, 5, 5, dtype=dtype)
        assert not tensor_vec8_supported(x)
        act = activations.ChannelPReLU(C).to(dtype)
        assert torch.equal(act(x), torch.nn.functional.prelu(x, act.weight))
        bn = torch.nn.BatchNorm2d(C).to(dtype)
        bn2 = torch.nn.BatchNorm2d(C).to(dtype)
        assert torch.equal(bn_act.fused_bn_act(x, bn, "relu"),
                           torch.relu(bn2(x)))
        mp = pool.FusedMaxPool2d(3, 2, 1)
        assert torch.equal(mp(x),
                           torch.nn.functional.max_pool2d(x, 3, 2, 1))


def test_the_four_ops_ask_the_one_predicate():
    assert activations.tensor_vec8_supported is tensor_vec8_supported
    assert bn_act.tensor_vec8_supported is tensor_vec8_supported
    assert pool.tensor_vec8_supported is tensor_vec8_supported
    assert _vec8.vec8_supported is vec8_supported
