"""The layer rows of tests/test_gpu_conv_f16s_routes.py: one per instantiation of conv_f16s_kernel, each the smallest layer that reaches it.
test_abi_and_host.py asks cf_conv2d_f16s_route for every row without a GPU; the GPU test asks it again with the real tensors and then
checks the numbers."""
from collections import namedtuple

PAD = {(3, 3): (1, 1), (1, 1): (0, 0), (1, 5): (0, 2), (5, 1): (2, 0)}

# tup: the instantiation <KH, KW, CK, WM, NTW, MAXT, NW, VEC, PRE, WL> the layer lands on.  view: the input is a view one float into a
# NaN-fenced buffer (data_ptr % 16 == 4): scalar staging at W % 4 == 0, the path the kernel documents for misaligned inputs.  nimg:
# images per workgroup (1: one sample per workgroup -> fused statistics).
Row = namedtuple("Row", "tup B C H W Cout k stride view nimg")
# SMALL_MAPS: the four-wave 3x3 vector shapes (and their PRE forms) take a stride-1 layer that WL declines while one image fills the 128-pixel
# tile.  WL declines when its 256-pixel tile holds two or more images after the staging budget (NIMG x (H+2) x (W+2) x 2 tasks <= 512), so
# an image needs 64 < H x W and (H+2) x (W+2) <= 128 with B >= 2: 6x12 (three images per 256-pixel tile, cut to two by the budget) or
# 10x8.  (8x12 is not enough: the budget cuts the 256-pixel tile to one image and WL takes the layer.)
ROWS = [
    # ---- 3x3, stride 1, weights through LDS (8 waves, 256-pixel tiles): not a 128-channel layer, one sample per workgroup, vector staging
    Row((3, 3, 16, 1, 1, 2, 8, 1, 0, 1), 2, 40, 20, 36, 24, (3, 3), 1, False, 1),    # Cout <= 32
    Row((3, 3, 16, 2, 2, 2, 8, 1, 0, 1), 2, 40, 20, 36, 48, (3, 3), 1, False, 1),    # 32 < Cout, not 128-wide
    # ---- 3x3, stride 1, register-fragment shapes (4 waves, 128-pixel tiles)
    Row((3, 3, 16, 2, 2, 2, 4, 1, 0, 0), 2, 40, 6, 12, 48, (3, 3), 1, False, 1),     # 6x12 maps, B >= 2: WL declines (see SMALL_MAPS)
    Row((3, 3, 16, 2, 2, 2, 4, 0, 0, 0), 2, 40, 20, 36, 48, (3, 3), 1, True, 1),     # misaligned input: WL and vector staging decline
    Row((3, 3, 16, 1, 1, 2, 4, 1, 0, 0), 3, 40, 10, 8, 20, (3, 3), 1, False, 1),     # Cout <= 32 on 10x8 maps: WL declines (see SMALL_MAPS)
    Row((3, 3, 16, 1, 1, 2, 4, 0, 0, 0), 11, 40, 4, 5, 20, (3, 3), 1, False, 6),     # W % 4 != 0; 4x5 maps: 6 images per workgroup, 6 + 5
    Row((3, 3, 16, 4, 4, 2, 4, 1, 0, 0), 128, 20, 32, 32, 128, (3, 3), 1, False, 1),  # Cout % 128 == 0 and >= 1024 workgroups: four waves
    Row((3, 3, 16, 4, 4, 2, 4, 0, 0, 0), 128, 20, 32, 32, 128, (3, 3), 1, True, 1),   # the same, misaligned input
    Row((3, 3, 16, 4, 2, 2, 8, 1, 0, 0), 2, 40, 32, 32, 128, (3, 3), 1, False, 1),   # Cout % 128 == 0, < 1024 workgroups: eight waves
    Row((3, 3, 16, 4, 2, 2, 8, 0, 0, 0), 11, 40, 4, 5, 128, (3, 3), 1, False, 6),    # the same at W % 4 != 0; 6 images per workgroup, 6 + 5
    # ---- 3x3, stride 2 (scalar staging only)
    Row((3, 3, 16, 1, 1, 5, 4, 0, 0, 0), 2, 40, 33, 45, 20, (3, 3), 2, False, 1),    # Cout <= 32, odd sizes, staging budget at MAXT = 5
    Row((3, 3, 16, 2, 1, 3, 4, 0, 0, 0), 7, 40, 8, 8, 64, (3, 3), 2, False, 4),      # 32 < Cout, not 128-wide; 4x4 outputs: 4 images, 4 + 3
    Row((3, 3, 16, 4, 2, 3, 4, 0, 0, 0), 2, 40, 30, 44, 224, (3, 3), 2, False, 1),   # 224 = 128 + 96: 128-channel blocks, last one 3/4 full
    # ---- 1x1 (scalar staging only)
    Row((1, 1, 32, 1, 1, 2, 4, 0, 0, 0), 5, 40, 6, 7, 24, (1, 1), 1, False, 3),      # Cout <= 32; 6x7 maps: 3 images per workgroup, 3 + 2
    Row((1, 1, 32, 2, 2, 2, 4, 0, 0, 0), 2, 72, 34, 50, 48, (1, 1), 2, False, 1),    # 32 < Cout, not 128-wide; stride 2
    Row((1, 1, 32, 4, 4, 2, 4, 0, 0, 0), 128, 40, 32, 32, 128, (1, 1), 1, False, 1),  # Cout % 128 == 0, >= 1024 workgroups: four waves
    Row((1, 1, 32, 4, 2, 2, 8, 0, 0, 0), 3, 40, 20, 28, 256, (1, 1), 1, False, 1),   # Cout % 128 == 0, < 1024 workgroups: eight waves
    # ---- 1x5 / 5x1 of the SepConvGRU (stride 1); VEC = 2: W % 4 == 0, aligned, within 2 tasks per thread
    Row((1, 5, 32, 2, 2, 4, 4, 2, 0, 0), 3, 40, 8, 8, 48, (1, 5), 1, False, 2),      # Cout % 128 != 0; 8x8 maps: 2 images per workgroup, 2 + 1
    Row((1, 5, 32, 2, 2, 4, 4, 0, 0, 0), 2, 40, 12, 30, 48, (1, 5), 1, False, 1),    # W % 4 != 0
    Row((1, 5, 32, 4, 2, 4, 8, 2, 0, 0), 2, 72, 12, 40, 128, (1, 5), 1, False, 1),   # Cout % 128 == 0: eight waves
    Row((1, 5, 32, 4, 2, 4, 8, 0, 0, 0), 3, 40, 8, 8, 128, (1, 5), 1, True, 2),      # misaligned input, 2 images per workgroup, 2 + 1
    Row((5, 1, 32, 2, 2, 4, 4, 2, 0, 0), 2, 40, 12, 40, 48, (5, 1), 1, False, 1),    # Cout % 128 != 0, 512 vector tasks (the budget)
    Row((5, 1, 32, 2, 2, 4, 4, 0, 0, 0), 3, 40, 8, 6, 48, (5, 1), 1, False, 2),      # W % 4 != 0; 8x6 maps: 2 images per workgroup, 2 + 1
    Row((5, 1, 32, 4, 2, 4, 8, 2, 0, 0), 3, 40, 8, 8, 128, (5, 1), 1, False, 2),     # Cout % 128 == 0; 2 images per workgroup, 2 + 1
    Row((5, 1, 32, 4, 2, 4, 8, 0, 0, 0), 2, 72, 12, 40, 128, (5, 1), 1, True, 1),    # misaligned input
]

# Maps one to three columns wide and taller than the scalar staging budget holds in one tile: f16s_plan gives the tile fewer rows (83 of a
# 130x1 map at 3x3 / stride 1: two tiles along y, the second part-filled).  Shapes the table above has already; the tile geometry is new.
NARROW_ROWS = [
    Row((3, 3, 16, 2, 2, 2, 4, 0, 0, 0), 2, 40, 130, 1, 48, (3, 3), 1, False, 1),    # 130x1: (128 + 2) x 3 records x 2 tasks > 2 x 256
    Row((3, 3, 16, 1, 1, 2, 4, 0, 0, 0), 2, 40, 70, 2, 20, (3, 3), 1, False, 1),     # 70x2: 64-row tiles, (64 + 2) x 4 x 2 > 512
    Row((3, 3, 16, 2, 1, 3, 4, 0, 0, 0), 2, 40, 135, 2, 64, (3, 3), 2, False, 1),    # stride 2, 68x1 outputs: (2 x 63 + 3) x 3 x 2 > 3 x 256
    Row((3, 3, 16, 1, 1, 5, 4, 0, 0, 0), 2, 40, 270, 1, 20, (3, 3), 2, False, 1),    # stride 2, Cout <= 32, 135x1 outputs
    Row((1, 5, 32, 2, 2, 4, 4, 0, 0, 0), 2, 40, 50, 3, 48, (1, 5), 1, False, 1),     # 1x5 on 50x3: 42 x (3 + 4) x 4 > 4 x 256
]

# deferred input normalisation (cf_conv2d_f16s_prenorm): 3x3, stride 1, vector staging, one sample per workgroup
PreRow = namedtuple("PreRow", "tup B C H W Cout")
PRE_ROWS = [
    PreRow((3, 3, 16, 1, 1, 2, 8, 1, 1, 1), 2, 40, 20, 36, 24),     # WL, Cout <= 32
    PreRow((3, 3, 16, 2, 2, 2, 8, 1, 1, 1), 2, 40, 20, 36, 48),     # WL, 64-channel
    PreRow((3, 3, 16, 2, 2, 2, 4, 1, 1, 0), 2, 40, 6, 12, 48),      # 6x12 maps, B >= 2: WL declines (see SMALL_MAPS)
    PreRow((3, 3, 16, 1, 1, 2, 4, 1, 1, 0), 3, 40, 10, 8, 20),      # 10x8 maps, Cout <= 32
    PreRow((3, 3, 16, 4, 4, 2, 4, 1, 1, 0), 128, 24, 32, 32, 128),  # Cout % 128 == 0, >= 1024 workgroups: four waves
]

# transposed 2x2 / stride 2 convolution: a 1x1 GEMM to 4 * Cout rows (co, dy, dx) with the scatter2x2 epilogue
ConvTRow = namedtuple("ConvTRow", "tup B Cin H W Cout nimg")
CONVT_ROWS = [
    ConvTRow((1, 1, 32, 1, 1, 2, 4, 0, 0, 0), 5, 40, 6, 7, 8, 3),       # 4 * Cout <= 32; 6x7 maps: 3 images per workgroup, 3 + 2
    ConvTRow((1, 1, 32, 2, 2, 2, 4, 0, 0, 0), 2, 72, 10, 20, 12, 1),    # 4 * Cout = 48
    ConvTRow((1, 1, 32, 4, 4, 2, 4, 0, 0, 0), 128, 40, 32, 32, 32, 1),  # 4 * Cout = 128, >= 1024 workgroups
    ConvTRow((1, 1, 32, 4, 2, 2, 8, 0, 0, 0), 2, 40, 16, 16, 32, 1),    # 4 * Cout = 128, < 1024 workgroups
]


def row_id(r):
    return "<%s>" % ",".join(map(str, r.tup)) + ("_view" if getattr(r, "view", False) else "") + ("_%dx%d" % (r.H, r.W) if r in NARROW_ROWS else "")
