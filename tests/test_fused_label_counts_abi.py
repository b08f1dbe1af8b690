"""
The fused warp + Dice entry points for label counts that are multiples of 4 but not 4 * 2^k (csrc/fused.hip: warp_dice_tile_pad,
the padded entry point of the kernel body it shares with warp_dice_tile): which kernel the library names, and that every other
count keeps its old answer.  Geometry only, no device needed.
"""

import neurite_amd as ne

N160 = ne._lib.ints([160] * 3)
POW2 = (4, 8, 16, 32, 64, 128, 256)
TUNES = (0, 1 << 30, 1 << 29, 3 | (3 << 4) | (4 << 8))


def name(L, store=0, tune=0, batch=4, mode=1):
    return ne._lib.lib().nrt_warp_dice_kernel_name(N160, N160, L, batch, mode, 0, store, 0, tune)


def test_padded_counts_name_their_own_kernel():
    pow2_names = {name(L, s, t, b, m) for L in POW2 for s in (0, 1) for t in TUNES for b in (1, 4) for m in (0, 1, 2)}
    assert b'' not in pow2_names
    for L in (12, 20, 24, 36, 252):
        for store in (0, 1):
            for tune in TUNES:
                for batch in (1, 4):
                    got = name(L, store, tune, batch)
                    assert got.startswith(b'warp_dice_tile_pad<'), (L, got)
                    assert got not in pow2_names, (L, got)
    # the lane group is the next power of two >= L / 4; L = 24 at 4 x 160^3 takes the x-march instance, tiles on request
    assert name(24) == b'warp_dice_tile_pad<8, 1, false, 3, float>'
    assert name(24, tune=3 | (3 << 4) | (4 << 8)) == b'warp_dice_tile_pad<8, 1, false, 1, float>'
    assert name(12, store=1) == b'warp_dice_tile_pad<4, 1, true, 1, float>'
    assert name(36) == b'warp_dice_tile_pad<16, 1, false, 1, float>'
    assert name(252) == b'warp_dice_tile_pad<64, 1, false, 1, float>'


def test_power_of_two_names_unchanged():
    assert name(32) in (b'warp_dice_tile<8, 1, false, 3, float>', b'warp_dice_wc<1, false, false, false, true, true>')
    assert name(32, tune=1 << 30) == b'warp_dice_tile<8, 1, false, 3, float>'
    assert name(32, tune=1 << 29) == b'warp_dice_wc<1, false, false, false, true, true>'
    assert name(16) == b'warp_dice_tile<4, 1, false, 1, float>'


def test_workspace_bytes():
    lib = ne._lib.lib()
    for L in (12, 20, 24, 36, 252):
        for tune in TUNES:
            assert lib.nrt_warp_dice_workspace_bytes(N160, L, 4, tune) > 0
    # it covers the partial rows of the launch: 3 L sums per row, on the geometry of the padded lane group
    assert lib.nrt_warp_dice_workspace_bytes(N160, 24, 4, 0) < lib.nrt_warp_dice_workspace_bytes(N160, 32, 4, 1 << 30)
    assert lib.nrt_warp_dice_workspace_bytes(N160, 3, 4, 0) == 0
    assert lib.nrt_warp_dice_workspace_bytes(N160, 6, 4, 0) == 0


def test_rejected_counts_stay_rejected():
    for L in (3, 5, 6, 260, 0, -4):
        for store in (0, 1):
            assert name(L, store) == b'', L
