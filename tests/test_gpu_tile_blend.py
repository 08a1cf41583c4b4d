'''fd_tile_blend_f32 on the device: bit for bit against the fp32 restatement of tile_ref.py on every grid of its table x every
(C, ld), feather, batch and affine, on the float4 and the scalar load path, inside guarded sentinel-filled buffers; a one-tile
grid against fd_nhwc_f32_to_nchw_f32; two launches against each other.'''
import numpy as np
import pytest
import torch

import tile_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64                                   # floats on either side of every output buffer (keeps 16-byte alignment)
SENTINEL = -7.0e33


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def guarded(shape, dev):
    '''(whole buffer, view of `shape` inside it): sentinel everywhere, GUARD floats around the view.'''
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    return whole, whole[GUARD:GUARD + n].view(shape)


def guards_intact(whole):
    w = whole.cpu()
    return bool((w[:GUARD] == SENTINEL).all()) and bool((w[-GUARD:] == SENTINEL).all())


def on_device(tiles, dev, misaligned=False):
    '''The tile rows in a device buffer; misaligned: the base 4 bytes off a 16-byte boundary, which must take the scalar
    loads whatever ld is.'''
    rows, ld = tiles.shape
    flat = torch.full((rows * ld + 4,), SENTINEL, dtype=torch.float32, device=dev)
    out = flat[1:1 + rows * ld].view(rows, ld) if misaligned else flat[:rows * ld].view(rows, ld)
    assert out.data_ptr() % 16 == (4 if misaligned else 0)
    out.copy_(tiles)
    return out


def blend(tiles_dev, B, C, grid, feather, affine, dev):
    from flexdiffuse_amd import ops
    H, W = grid[:2]
    whole, out = guarded((B, C, H, W), dev)
    a, b, clamp = affine
    ops.tile_blend(tiles_dev, B, C, R.grid_args(grid), feather, a, b, clamp, out=out)
    got = out.cpu()
    assert guards_intact(whole), (grid, B, C, feather)
    assert not bool((got == SENTINEL).any()), (grid, B, C, feather)          # every element is written
    return got


@pytest.mark.parametrize('grid', R.GRIDS)
def test_tile_blend_kernel_vs_restatement(dev, grid):
    n = 0
    for B, (C, ld), feather, affine in R.cases(grid):
        tiles = R.inputs(grid, B, ld)
        want = R.blend_ref(tiles, B, C, ld, grid, feather, *affine)
        got = blend(on_device(tiles, dev), B, C, grid, feather, affine, dev)
        assert torch.equal(got, want), (grid, B, C, ld, feather, affine, float((got - want).abs().max()))
        n += 1
    assert n == 2 * len(R.CHANNELS) * 5 * 2


@pytest.mark.parametrize('grid', R.GRIDS)
def test_tile_blend_misaligned_base_takes_the_scalar_path(dev, grid):
    '''ld 4 and 8 from a base one float off a 16-byte boundary: the same bits as the aligned launch and the restatement.'''
    for B, (C, ld) in ((1, (3, 4)), (2, (8, 8)), (2, (5, 8))):
        for feather in R.feathers(grid)[1:3]:
            affine = R.AFFINES[B - 1]
            tiles = R.inputs(grid, B, ld, seed=1)
            want = R.blend_ref(tiles, B, C, ld, grid, feather, *affine)
            got = blend(on_device(tiles, dev, misaligned=True), B, C, grid, feather, affine, dev)
            assert torch.equal(got, want), (grid, B, C, ld, feather)
            assert torch.equal(got, blend(on_device(tiles, dev), B, C, grid, feather, affine, dev))


@pytest.mark.parametrize('affine', [(0.5, 0.5, True), (1.0, 0.0, False)])
def test_one_tile_equals_nhwc_to_nchw(dev, affine):
    '''With a a power of two the product is exact, so a one-tile grid gives the bits of fd_nhwc_f32_to_nchw_f32 on the same
    rows whichever way that kernel's x * a + b is contracted.'''
    from flexdiffuse_amd import ops
    a, b, clamp = affine
    for (H, W), (C, ld), B in (((8, 8), (3, 4), 2), ((6, 10), (8, 8), 1), ((5, 7), (3, 3), 2)):
        grid = (H, W, H, W, H, W)
        tiles = on_device(R.inputs(grid, B, ld), dev)
        want = ops.nhwc_to_nchw(tiles, B, C, H, W, a, b, clamp).cpu()
        for feather in ((1, 1), (3, 2)):
            assert torch.equal(blend(tiles, B, C, grid, feather, affine, dev), want), (H, W, C, ld, feather)


def test_two_launches_give_equal_bits(dev):
    grid, B, C, ld = R.GRIDS[3], 2, 3, 4
    tiles = on_device(R.inputs(grid, B, ld), dev)
    first = blend(tiles, B, C, grid, (2, 2), R.AFFINES[1], dev)
    assert torch.equal(first, blend(tiles, B, C, grid, (2, 2), R.AFFINES[1], dev))
    assert torch.equal(tiles.cpu(), R.inputs(grid, B, ld))                   # the tiles are only read


def test_tile_blend_plan_replay(dev):
    '''The entry point records itself into a launch plan like its siblings: the replay writes the same bits.'''
    from flexdiffuse_amd import hip, ops
    grid, B, C, ld = R.GRIDS[2], 2, 3, 4
    tiles = on_device(R.inputs(grid, B, ld), dev)
    whole, out = guarded((B, C) + grid[:2], dev)
    plan = hip.Plan()
    with plan.record():
        ops.tile_blend(tiles, B, C, R.grid_args(grid), (2, 2), 0.5, 0.5, True, out=out)
    assert len(plan) == 1
    want = out.cpu()
    out.fill_(SENTINEL)
    plan.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), want) and guards_intact(whole)
    assert torch.equal(want, R.blend_ref(R.inputs(grid, B, ld), B, C, ld, grid, (2, 2), 0.5, 0.5, True))
