"""Case tables of tests/test_gpu_gemm_f32.py: the fp32 GEMM (gemm_f32_kernel, flow_kernels.hip)
behind idf_conv1x1_f32, idf_conv3x3_f32 and idf_conv3x3_fold_f32.

tests/test_host_logic.py checks the tables against the dispatch itself (idf_gemm_launch_info, on
the host): that the dense rows reach every tile width and both arms of the block remap, and which
row count first selects each taller row tile."""
from collections import namedtuple

BNS = (16, 32, 48, 64, 128)
# every (BM, BN) launch_bn can pick: BM 64 / 128 / 256, and no 256 x 128 tile
ALL_TILES = frozenset((bm, bn) for bn in BNS for bm in (64, 128, 256) if (bm, bn) != (256, 128))
# the grid size from which the dispatcher takes a taller row tile (4 blocks per CU)
MIN_BLOCKS = 1024

Dense = namedtuple("Dense", "N K P")
# N: each BN, a ragged last tile, both arms of the 64-vs-128 choice (130 -> 64, 65 / 200 -> 128)
# K: below one chunk (4), a multiple of 4 but not of 16 (20, 36, 132), whole chunks (16)
# P: one row, ragged row tiles, grids of fewer than 8 blocks and of no multiple of 8 blocks
DENSE_N = (1, 16, 17, 32, 33, 48, 49, 64, 65, 130, 200)
DENSE_K = (4, 20, 16, 36, 132)
DENSE_P = (1, 63, 65, 200, 1000)
DENSE = [
    Dense(1, 4, 1), Dense(16, 20, 63), Dense(17, 16, 65), Dense(32, 36, 200),
    Dense(33, 132, 1000), Dense(48, 4, 1000), Dense(49, 20, 200), Dense(64, 16, 65),
    Dense(65, 36, 63), Dense(130, 132, 1), Dense(200, 20, 1000), Dense(16, 132, 200),
    Dense(32, 4, 65), Dense(48, 36, 1), Dense(64, 132, 63), Dense(1, 16, 1000),
    Dense(200, 36, 65), Dense(130, 4, 200), Dense(17, 20, 1), Dense(65, 16, 1000),
    Dense(130, 20, 1000),
]

# the widest N of each tile width: the BM rows of the table run these
WIDEST_N = {16: 16, 32: 32, 48: 48, 64: 64, 128: 128}
BM_K = 20
BM_RAGGED = 37  # rows past the threshold, so the last row tile is partly filled


def first_p(bm, n_tiles):
    """The smallest P whose grid of BM-row tiles has MIN_BLOCKS blocks (the rule restated for
    the host test, which compares it with what idf_gemm_launch_info reports)."""
    m = -(-MIN_BLOCKS // n_tiles)  # row tiles needed
    return bm * (m - 1) + 1


Conv3 = namedtuple("Conv3", "B H W C N act")
CONV3 = [
    Conv3(3, 2, 3, 4, 8, "ReLU"),       # every pixel a border pixel
    Conv3(2, 1, 5, 8, 16, "None"),      # H = 1
    Conv3(2, 5, 1, 8, 16, "ReLU"),      # W = 1
    Conv3(3, 7, 5, 20, 40, "ReLU"),     # 35 pixels an image: a 64-row tile spans two images
    Conv3(2, 3, 3, 12, 44, "None"),     # one interior pixel
    Conv3(1, 16, 16, 36, 44, "ReLU"),
    Conv3(2, 27, 23, 40, 32, "LeakyReLU"),
]
# large P: (H, W, C, N) at which B = 64 launches BM = 256; the BM = 128 batch comes from the info
CONV3_LARGE = (64, 64, 4, 16)
CONV3_LARGE_B256 = 64

# epilogues
EPI_GEOM = (3, 5, 7)  # B, H, W: P = 105
EPI_K = 36
COUPLE_N = (6, 20)
PRIOR_N_MEAN = (3, 12, 24)
# whole blocks on the plain path
BLOCK_GEOM = (2, 7, 5)
BLOCK_DEPTH = 3
