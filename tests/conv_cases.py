"""The bf16 conv kernel variants (`kVariants[]`, csrc/sat_conv_glds.hip) as one table of test cases: every variant in every
mode its predicate admits, at geometries with the tails where kernels go wrong.  A plain helper module (like ss_reference.py).

`sat_conv_glds_launch` replaces a variant the op cannot run by the built-in choice and still returns SAT_OK, so a test that
names a variant proves nothing about that kernel unless it asks `sat_conv_resolved_variant` first: `run_named` does.  The
table is checked WITHOUT a GPU (tests/test_conv_cases_host.py: every row resolves to the variant it names, the table is
complete) and run on one (tests/test_gpu_conv_variants.py: every row against the f64 definition and its bit family).
"""
import ctypes as C
import importlib

sat = importlib.import_module("show-and-tell_amd")
L = sat._lib

# ---- the kernel families of kVariants[] and the modes their predicates admit (variant_ok and the *_ok functions) ----
# ring variants: (tile columns BN, ring stages S, waves, wave-specialised, fragment prefetch, tile rows BM)
RING_PARAMS = {
    1: (128, 4, 8, 0, 0, 128), 2: (128, 3, 8, 0, 0, 128), 3: (128, 2, 8, 0, 0, 128), 4: (64, 4, 8, 0, 0, 128), 5: (64, 3, 8, 0, 0, 128),
    6: (64, 2, 8, 0, 0, 128), 7: (128, 4, 4, 0, 0, 128), 8: (128, 2, 4, 0, 0, 128), 9: (64, 3, 4, 0, 0, 128), 10: (64, 2, 4, 0, 0, 128),
    11: (128, 4, 8, 1, 0, 128), 12: (128, 3, 8, 1, 0, 128), 13: (128, 2, 8, 1, 0, 128), 14: (64, 4, 8, 1, 0, 128), 15: (64, 3, 8, 1, 0, 128),
    16: (128, 4, 8, 1, 1, 128), 17: (128, 4, 8, 0, 1, 128), 18: (128, 4, 4, 0, 1, 128), 19: (64, 4, 8, 1, 1, 128), 20: (64, 4, 8, 0, 1, 128),
    21: (64, 4, 4, 0, 1, 128), 22: (256, 2, 8, 0, 0, 128), 23: (256, 3, 8, 0, 0, 128), 24: (256, 3, 8, 0, 0, 64), 25: (128, 3, 8, 0, 0, 64),
    26: (128, 2, 8, 0, 0, 64)}
FAMILIES = {
    "ring": [v for v, p in RING_PARAMS.items() if not (p[3] or p[4]) and p[5] == 128],     # unified waves, 128-row tiles
    "ring_spec_pf": [v for v, p in RING_PARAMS.items() if p[3] or p[4]],                  # no in-LDS input transform
    "ring_bm64": [v for v, p in RING_PARAMS.items() if p[5] == 64],                       # no statistics slabs (they are 128-row tiles)
    "xp": [27, 28, 29], "pr": [30], "stem": [31], "pw": [32], "aw": [33, 34], "ap": [35], "ay": [36, 37],
    "rs": [38], "rs64": [39], "rs8": [40], "rs_stem": [41]}
STATS = ("slab", "atomic", "none")                  # per-tile slabs, integer-atomic sums, no statistics
EVAL = ("eval", "eval_res")                         # inference epilogue: affine + ReLU, affine + residual + ReLU
BN = ("bn_table", "bn_derive")                      # fused input BatchNorm + ReLU: table given / derived from the producer's sums
ADMITS = {
    "ring": STATS + EVAL + BN, "ring_spec_pf": STATS + EVAL, "ring_bm64": ("atomic", "none") + EVAL + BN,
    "xp": STATS + BN, "pr": STATS + BN, "stem": STATS, "pw": STATS + ("eval",) + BN, "aw": STATS + EVAL + BN, "ap": STATS + BN,
    "ay": ("ay_table", "ay_derive"),                # operand = relu(bn(in0) + in1), also written to out1 (SAT_CONV_IN_RESIDUAL)
    "rs": STATS + ("eval",), "rs64": STATS + ("eval",), "rs8": STATS + ("eval",), "rs_stem": STATS + ("eval",)}
NEEDS_PACKED = FAMILIES["pw"] + FAMILIES["aw"] + FAMILIES["ap"] + FAMILIES["ay"]
# rows whose predicate reads a device property: none -- rs64_grid, rs_stem_grid and ap_workers are functions of the geometry
GPU_ONLY_ROWS = []


def family_of(variant):
    return next(f for f, vs in FAMILIES.items() if variant in vs)


# ---- geometries.  dense: NHWC input [N][H][W][Cin], kernel (KH, KW), padding (pad, padw); stem: the op program's stem layout, a
# 7 x 1 kernel over rows of 8 pixels x 4 channels of an [N][H][W][4] image (Cin = 32, pixel stride 4 elements), H / W the padded
# image, Hout / Wout given.  ldc: row stride of the output (and of the residual), 0 = Cout ----
def _g(N, H, W, Cin, Cout, KH=1, KW=1, stride=1, pad=0, padw=None, ldc=0, layout="dense", Hout=0, Wout=0):
    padw = pad if padw is None else padw
    if layout == "dense":
        Hout, Wout = (H + 2 * pad - KH) // stride + 1, (W + 2 * padw - KW) // stride + 1
    return dict(N=N, H=H, W=W, Cin=Cin, Cout=Cout, KH=KH, KW=KW, stride=stride, pad=pad, padw=padw, ldc=ldc, layout=layout,
                Hout=Hout, Wout=Wout, M=N * Hout * Wout, K=KH * KW * Cin)


GEOS = {
    # ring kernel: M = 585 (ragged for 128- and 64-row tiles), Cout = 192 (ragged for 128- and 256-column tiles), 9 K-steps
    "r3x3": _g(3, 15, 13, 64, 192, 3, 3, 1, 1),
    # 5 K-steps (no multiple of a ring depth), Cout = 136: a ragged last column tile at every tile width
    "r1x1_k5": _g(5, 8, 8, 320, 136),
    # one K-step: shorter than every ring
    "r1x1_k1": _g(2, 9, 11, 64, 200),
    # Cin % 64 != 0 (the non-uniform ring path), stride 2, 4 K-steps with a ragged last one
    "r_c24_s2": _g(2, 9, 9, 24, 200, 3, 3, 2, 1),
    # rectangular kernel, padding on one axis only (SAT_CONV_PADW), 7 K-steps
    "r_1x7": _g(2, 10, 12, 64, 136, 1, 7, 1, 0, 3),
    # two K-steps; 264 columns: a ragged last column tile BEHIND full ones at every tile width; M = 130
    "r_n264": _g(1, 10, 13, 128, 264),
    # output rows longer than Cout: the channels next to the tile stay untouched
    "r_ldc": _g(2, 9, 11, 64, 136, 3, 3, 1, 1, ldc=200),
    # expansion 1x1 (K = 256 / 128 / 64), ragged M
    "x_k256": _g(5, 12, 12, 256, 512), "x_k128": _g(3, 7, 9, 128, 512), "x_k64": _g(3, 9, 11, 64, 512),
    # conv_ap_kernel persistent over two row tiles per worker (259 row tiles, the last one ragged)
    "ap_big": _g(10, 58, 57, 256, 128),
    # 3x3 / stride 1 / pad 1 patch kernels: rows of several images in a tile, the widest image (W = 31), a ragged column tile
    "p_w13": _g(3, 15, 13, 64, 256, 3, 3, 1, 1), "p_w31": _g(2, 5, 31, 128, 128, 3, 3, 1, 1), "p_n136": _g(2, 7, 7, 128, 136, 3, 3, 1, 1),
    # 1x1 with the weights in registers: 8 K-steps, ragged M; stride 2
    "a_k512": _g(3, 9, 13, 512, 256), "a_s2": _g(2, 15, 13, 128, 256, 1, 1, 2, 0),
    # stem layout (stride 2: a 16-byte chunk is two pixels): 64-pixel output rows, 32.5 row tiles; ResNet's stem at 224 x 224, six
    # images: the smallest batch with as many statistics slabs (588) as conv_rs_stem_kernel has workgroups (512)
    "s_w64": _g(1, 136, 136, 32, 64, 7, 1, 2, 0, layout="stem", Hout=65, Wout=64),
    "s_224": _g(6, 230, 232, 32, 64, 7, 1, 2, 0, layout="stem", Hout=112, Wout=112),
    # rolling-window kernels: 32 channels without / with padding, 64 -> 64 on short rows, stride 2 over 8 channels
    "rs_p0": _g(1, 6, 132, 32, 32, 3, 3, 1, 0), "rs_p1": _g(2, 3, 128, 32, 64, 3, 3, 1, 1),
    "rs64_w50": _g(1, 4, 50, 64, 64, 3, 3, 1, 1), "rs64_w64": _g(3, 4, 64, 64, 64, 3, 3, 1, 1),
    "rs8_w130": _g(1, 7, 261, 8, 32, 3, 3, 2, 0),
}

# ---- the rows: (variant, mode, geometry) ----
CASES = [
    (1, "slab", "r3x3"), (1, "slab", "r1x1_k5"), (1, "slab", "r1x1_k1"), (1, "slab", "r_c24_s2"), (1, "slab", "r_1x7"),
    (1, "slab", "r_n264"), (1, "atomic", "r3x3"), (1, "none", "r3x3"), (1, "eval", "r3x3"), (1, "eval_res", "r3x3"),
    (1, "bn_table", "r1x1_k5"), (1, "bn_derive", "r1x1_k5"), (1, "none", "r_ldc"), (1, "eval_res", "r_ldc"),
    (1, "slab", "x_k256"), (1, "atomic", "x_k256"), (1, "none", "x_k256"), (1, "bn_table", "x_k256"),
    (1, "bn_derive", "x_k256"), (1, "slab", "x_k128"), (1, "slab", "x_k64"), (1, "slab", "ap_big"), (1, "eval", "p_w13"),
    (1, "slab", "p_w13"), (1, "atomic", "p_w13"), (1, "none", "p_w13"), (1, "slab", "p_w31"), (1, "slab", "p_n136"),
    (1, "slab", "a_k512"), (1, "atomic", "a_k512"), (1, "none", "a_k512"), (1, "eval", "a_k512"), (1, "eval_res", "a_k512"),
    (1, "bn_table", "a_k512"), (1, "bn_derive", "a_k512"), (1, "slab", "a_s2"), (2, "slab", "r3x3"), (2, "slab", "r1x1_k5"),
    (2, "slab", "r1x1_k1"), (2, "slab", "r_c24_s2"), (2, "slab", "r_1x7"), (2, "slab", "r_n264"), (2, "atomic", "r3x3"),
    (2, "none", "r3x3"), (2, "eval", "r3x3"), (2, "eval_res", "r3x3"), (2, "bn_table", "r1x1_k5"), (2, "bn_derive", "r1x1_k5"),
    (2, "none", "r_ldc"), (2, "eval_res", "r_ldc"), (3, "slab", "r3x3"), (3, "slab", "r1x1_k5"), (3, "slab", "r1x1_k1"),
    (3, "slab", "r_c24_s2"), (3, "slab", "r_1x7"), (3, "slab", "r_n264"), (3, "atomic", "r3x3"), (3, "none", "r3x3"),
    (3, "eval", "r3x3"), (3, "eval_res", "r3x3"), (3, "bn_table", "r1x1_k5"), (3, "bn_derive", "r1x1_k5"), (3, "none", "r_ldc"),
    (3, "eval_res", "r_ldc"), (3, "slab", "x_k256"), (3, "atomic", "x_k256"), (3, "none", "x_k256"), (3, "bn_table", "x_k256"),
    (3, "bn_derive", "x_k256"), (4, "slab", "r3x3"), (4, "slab", "r1x1_k5"), (4, "slab", "r1x1_k1"), (4, "slab", "r_c24_s2"),
    (4, "slab", "r_1x7"), (4, "slab", "r_n264"), (4, "atomic", "r3x3"), (4, "none", "r3x3"), (4, "eval", "r3x3"),
    (4, "eval_res", "r3x3"), (4, "bn_table", "r1x1_k5"), (4, "bn_derive", "r1x1_k5"), (4, "none", "r_ldc"),
    (4, "eval_res", "r_ldc"), (5, "slab", "r3x3"), (5, "slab", "r1x1_k5"), (5, "slab", "r1x1_k1"), (5, "slab", "r_c24_s2"),
    (5, "slab", "r_1x7"), (5, "slab", "r_n264"), (5, "atomic", "r3x3"), (5, "none", "r3x3"), (5, "eval", "r3x3"),
    (5, "eval_res", "r3x3"), (5, "bn_table", "r1x1_k5"), (5, "bn_derive", "r1x1_k5"), (5, "none", "r_ldc"),
    (5, "eval_res", "r_ldc"), (5, "slab", "rs_p0"), (5, "atomic", "rs_p0"), (5, "none", "rs_p0"), (5, "eval", "rs_p0"),
    (5, "slab", "rs_p1"), (5, "slab", "rs64_w50"), (5, "atomic", "rs64_w50"), (5, "none", "rs64_w50"), (5, "eval", "rs64_w50"),
    (5, "slab", "rs64_w64"), (5, "slab", "rs8_w130"), (5, "atomic", "rs8_w130"), (5, "none", "rs8_w130"),
    (5, "eval", "rs8_w130"), (6, "slab", "r3x3"), (6, "slab", "r1x1_k5"), (6, "slab", "r1x1_k1"), (6, "slab", "r_c24_s2"),
    (6, "slab", "r_1x7"), (6, "slab", "r_n264"), (6, "atomic", "r3x3"), (6, "none", "r3x3"), (6, "eval", "r3x3"),
    (6, "eval_res", "r3x3"), (6, "bn_table", "r1x1_k5"), (6, "bn_derive", "r1x1_k5"), (6, "none", "r_ldc"),
    (6, "eval_res", "r_ldc"), (7, "slab", "r3x3"), (7, "slab", "r1x1_k5"), (7, "slab", "r1x1_k1"), (7, "slab", "r_c24_s2"),
    (7, "slab", "r_1x7"), (7, "slab", "r_n264"), (7, "atomic", "r3x3"), (7, "none", "r3x3"), (7, "eval", "r3x3"),
    (7, "eval_res", "r3x3"), (7, "bn_table", "r1x1_k5"), (7, "bn_derive", "r1x1_k5"), (7, "none", "r_ldc"),
    (7, "eval_res", "r_ldc"), (8, "slab", "r3x3"), (8, "slab", "r1x1_k5"), (8, "slab", "r1x1_k1"), (8, "slab", "r_c24_s2"),
    (8, "slab", "r_1x7"), (8, "slab", "r_n264"), (8, "atomic", "r3x3"), (8, "none", "r3x3"), (8, "eval", "r3x3"),
    (8, "eval_res", "r3x3"), (8, "bn_table", "r1x1_k5"), (8, "bn_derive", "r1x1_k5"), (8, "none", "r_ldc"),
    (8, "eval_res", "r_ldc"), (9, "slab", "r3x3"), (9, "slab", "r1x1_k5"), (9, "slab", "r1x1_k1"), (9, "slab", "r_c24_s2"),
    (9, "slab", "r_1x7"), (9, "slab", "r_n264"), (9, "atomic", "r3x3"), (9, "none", "r3x3"), (9, "eval", "r3x3"),
    (9, "eval_res", "r3x3"), (9, "bn_table", "r1x1_k5"), (9, "bn_derive", "r1x1_k5"), (9, "none", "r_ldc"),
    (9, "eval_res", "r_ldc"), (10, "slab", "r3x3"), (10, "slab", "r1x1_k5"), (10, "slab", "r1x1_k1"), (10, "slab", "r_c24_s2"),
    (10, "slab", "r_1x7"), (10, "slab", "r_n264"), (10, "atomic", "r3x3"), (10, "none", "r3x3"), (10, "eval", "r3x3"),
    (10, "eval_res", "r3x3"), (10, "bn_table", "r1x1_k5"), (10, "bn_derive", "r1x1_k5"), (10, "none", "r_ldc"),
    (10, "eval_res", "r_ldc"), (10, "slab", "s_w64"), (10, "atomic", "s_w64"), (10, "none", "s_w64"), (10, "slab", "s_224"),
    (10, "eval", "s_w64"), (11, "slab", "r3x3"), (11, "slab", "r1x1_k5"), (11, "slab", "r1x1_k1"), (11, "slab", "r_c24_s2"),
    (11, "slab", "r_1x7"), (11, "slab", "r_n264"), (11, "atomic", "r3x3"), (11, "none", "r3x3"), (11, "eval", "r3x3"),
    (11, "eval_res", "r3x3"), (11, "none", "r_ldc"), (11, "eval_res", "r_ldc"), (12, "slab", "r3x3"), (12, "slab", "r1x1_k5"),
    (12, "slab", "r1x1_k1"), (12, "slab", "r_c24_s2"), (12, "slab", "r_1x7"), (12, "slab", "r_n264"), (12, "atomic", "r3x3"),
    (12, "none", "r3x3"), (12, "eval", "r3x3"), (12, "eval_res", "r3x3"), (12, "none", "r_ldc"), (12, "eval_res", "r_ldc"),
    (13, "slab", "r3x3"), (13, "slab", "r1x1_k5"), (13, "slab", "r1x1_k1"), (13, "slab", "r_c24_s2"), (13, "slab", "r_1x7"),
    (13, "slab", "r_n264"), (13, "atomic", "r3x3"), (13, "none", "r3x3"), (13, "eval", "r3x3"), (13, "eval_res", "r3x3"),
    (13, "none", "r_ldc"), (13, "eval_res", "r_ldc"), (14, "slab", "r3x3"), (14, "slab", "r1x1_k5"), (14, "slab", "r1x1_k1"),
    (14, "slab", "r_c24_s2"), (14, "slab", "r_1x7"), (14, "slab", "r_n264"), (14, "atomic", "r3x3"), (14, "none", "r3x3"),
    (14, "eval", "r3x3"), (14, "eval_res", "r3x3"), (14, "none", "r_ldc"), (14, "eval_res", "r_ldc"), (15, "slab", "r3x3"),
    (15, "slab", "r1x1_k5"), (15, "slab", "r1x1_k1"), (15, "slab", "r_c24_s2"), (15, "slab", "r_1x7"), (15, "slab", "r_n264"),
    (15, "atomic", "r3x3"), (15, "none", "r3x3"), (15, "eval", "r3x3"), (15, "eval_res", "r3x3"), (15, "none", "r_ldc"),
    (15, "eval_res", "r_ldc"), (16, "slab", "r3x3"), (16, "slab", "r1x1_k5"), (16, "slab", "r1x1_k1"), (16, "slab", "r_c24_s2"),
    (16, "slab", "r_1x7"), (16, "slab", "r_n264"), (16, "atomic", "r3x3"), (16, "none", "r3x3"), (16, "eval", "r3x3"),
    (16, "eval_res", "r3x3"), (16, "none", "r_ldc"), (16, "eval_res", "r_ldc"), (17, "slab", "r3x3"), (17, "slab", "r1x1_k5"),
    (17, "slab", "r1x1_k1"), (17, "slab", "r_c24_s2"), (17, "slab", "r_1x7"), (17, "slab", "r_n264"), (17, "atomic", "r3x3"),
    (17, "none", "r3x3"), (17, "eval", "r3x3"), (17, "eval_res", "r3x3"), (17, "none", "r_ldc"), (17, "eval_res", "r_ldc"),
    (18, "slab", "r3x3"), (18, "slab", "r1x1_k5"), (18, "slab", "r1x1_k1"), (18, "slab", "r_c24_s2"), (18, "slab", "r_1x7"),
    (18, "slab", "r_n264"), (18, "atomic", "r3x3"), (18, "none", "r3x3"), (18, "eval", "r3x3"), (18, "eval_res", "r3x3"),
    (18, "none", "r_ldc"), (18, "eval_res", "r_ldc"), (19, "slab", "r3x3"), (19, "slab", "r1x1_k5"), (19, "slab", "r1x1_k1"),
    (19, "slab", "r_c24_s2"), (19, "slab", "r_1x7"), (19, "slab", "r_n264"), (19, "atomic", "r3x3"), (19, "none", "r3x3"),
    (19, "eval", "r3x3"), (19, "eval_res", "r3x3"), (19, "none", "r_ldc"), (19, "eval_res", "r_ldc"), (20, "slab", "r3x3"),
    (20, "slab", "r1x1_k5"), (20, "slab", "r1x1_k1"), (20, "slab", "r_c24_s2"), (20, "slab", "r_1x7"), (20, "slab", "r_n264"),
    (20, "atomic", "r3x3"), (20, "none", "r3x3"), (20, "eval", "r3x3"), (20, "eval_res", "r3x3"), (20, "none", "r_ldc"),
    (20, "eval_res", "r_ldc"), (21, "slab", "r3x3"), (21, "slab", "r1x1_k5"), (21, "slab", "r1x1_k1"), (21, "slab", "r_c24_s2"),
    (21, "slab", "r_1x7"), (21, "slab", "r_n264"), (21, "atomic", "r3x3"), (21, "none", "r3x3"), (21, "eval", "r3x3"),
    (21, "eval_res", "r3x3"), (21, "none", "r_ldc"), (21, "eval_res", "r_ldc"), (22, "slab", "r3x3"), (22, "slab", "r1x1_k5"),
    (22, "slab", "r1x1_k1"), (22, "slab", "r_c24_s2"), (22, "slab", "r_1x7"), (22, "slab", "r_n264"), (22, "atomic", "r3x3"),
    (22, "none", "r3x3"), (22, "eval", "r3x3"), (22, "eval_res", "r3x3"), (22, "bn_table", "r1x1_k5"),
    (22, "bn_derive", "r1x1_k5"), (22, "none", "r_ldc"), (22, "eval_res", "r_ldc"), (23, "slab", "r3x3"),
    (23, "slab", "r1x1_k5"), (23, "slab", "r1x1_k1"), (23, "slab", "r_c24_s2"), (23, "slab", "r_1x7"), (23, "slab", "r_n264"),
    (23, "atomic", "r3x3"), (23, "none", "r3x3"), (23, "eval", "r3x3"), (23, "eval_res", "r3x3"), (23, "bn_table", "r1x1_k5"),
    (23, "bn_derive", "r1x1_k5"), (23, "none", "r_ldc"), (23, "eval_res", "r_ldc"), (24, "atomic", "r3x3"),
    (24, "atomic", "r1x1_k5"), (24, "atomic", "r1x1_k1"), (24, "atomic", "r_c24_s2"), (24, "atomic", "r_1x7"),
    (24, "atomic", "r_n264"), (24, "none", "r3x3"), (24, "eval", "r3x3"), (24, "eval_res", "r3x3"), (24, "bn_table", "r1x1_k5"),
    (24, "bn_derive", "r1x1_k5"), (24, "none", "r_ldc"), (24, "eval_res", "r_ldc"), (25, "atomic", "r3x3"),
    (25, "atomic", "r1x1_k5"), (25, "atomic", "r1x1_k1"), (25, "atomic", "r_c24_s2"), (25, "atomic", "r_1x7"),
    (25, "atomic", "r_n264"), (25, "none", "r3x3"), (25, "eval", "r3x3"), (25, "eval_res", "r3x3"), (25, "bn_table", "r1x1_k5"),
    (25, "bn_derive", "r1x1_k5"), (25, "none", "r_ldc"), (25, "eval_res", "r_ldc"), (26, "atomic", "r3x3"),
    (26, "atomic", "r1x1_k5"), (26, "atomic", "r1x1_k1"), (26, "atomic", "r_c24_s2"), (26, "atomic", "r_1x7"),
    (26, "atomic", "r_n264"), (26, "none", "r3x3"), (26, "eval", "r3x3"), (26, "eval_res", "r3x3"), (26, "bn_table", "r1x1_k5"),
    (26, "bn_derive", "r1x1_k5"), (26, "none", "r_ldc"), (26, "eval_res", "r_ldc"), (27, "slab", "x_k256"),
    (27, "atomic", "x_k256"), (27, "none", "x_k256"), (27, "bn_table", "x_k256"), (27, "bn_derive", "x_k256"),
    (27, "slab", "x_k128"), (27, "slab", "x_k64"), (27, "slab", "ap_big"), (28, "slab", "x_k256"), (28, "atomic", "x_k256"),
    (28, "none", "x_k256"), (28, "bn_table", "x_k256"), (28, "bn_derive", "x_k256"), (28, "slab", "x_k128"),
    (28, "slab", "x_k64"), (29, "slab", "x_k256"), (29, "atomic", "x_k256"), (29, "none", "x_k256"), (29, "bn_table", "x_k256"),
    (29, "bn_derive", "x_k256"), (29, "slab", "x_k128"), (29, "slab", "x_k64"), (30, "slab", "p_w13"), (30, "atomic", "p_w13"),
    (30, "none", "p_w13"), (30, "bn_table", "p_w13"), (30, "bn_derive", "p_w13"), (30, "slab", "p_w31"), (30, "slab", "p_n136"),
    (30, "none", "r_ldc"), (31, "slab", "s_w64"), (31, "atomic", "s_w64"), (31, "none", "s_w64"), (31, "slab", "s_224"),
    (32, "slab", "p_w13"), (32, "atomic", "p_w13"), (32, "none", "p_w13"), (32, "bn_table", "p_w13"),
    (32, "bn_derive", "p_w13"), (32, "eval", "p_w13"), (32, "slab", "p_w31"), (33, "slab", "ap_big"), (33, "slab", "a_k512"),
    (33, "atomic", "a_k512"), (33, "none", "a_k512"), (33, "eval", "a_k512"), (33, "eval_res", "a_k512"),
    (33, "bn_table", "a_k512"), (33, "bn_derive", "a_k512"), (33, "slab", "a_s2"), (33, "slab", "x_k64"),
    (34, "slab", "a_k512"), (34, "atomic", "a_k512"), (34, "none", "a_k512"), (34, "eval", "a_k512"),
    (34, "eval_res", "a_k512"), (34, "bn_table", "a_k512"), (34, "bn_derive", "a_k512"), (34, "slab", "a_s2"),
    (34, "slab", "x_k64"), (35, "slab", "x_k256"), (35, "atomic", "x_k256"), (35, "none", "x_k256"), (35, "bn_table", "x_k256"),
    (35, "bn_derive", "x_k256"), (35, "slab", "ap_big"), (36, "ay_table", "a_k512"), (36, "ay_derive", "a_k512"),
    (37, "ay_table", "a_k512"), (37, "ay_derive", "a_k512"), (38, "slab", "rs_p0"), (38, "atomic", "rs_p0"),
    (38, "none", "rs_p0"), (38, "eval", "rs_p0"), (38, "slab", "rs_p1"), (39, "slab", "rs64_w50"), (39, "atomic", "rs64_w50"),
    (39, "none", "rs64_w50"), (39, "eval", "rs64_w50"), (39, "slab", "rs64_w64"), (40, "slab", "rs8_w130"),
    (40, "atomic", "rs8_w130"), (40, "none", "rs8_w130"), (40, "eval", "rs8_w130"), (41, "slab", "s_224"),
    (41, "atomic", "s_w64"), (41, "none", "s_w64"), (41, "eval", "s_w64"),
]


def expected_pairs():
    """every (variant, mode) the family table admits"""
    return {(v, m) for f, vs in FAMILIES.items() for v in vs for m in ADMITS[f]}


def check_complete(cases=None):
    """the rows cover every variant in every admitted mode, and name nothing else"""
    have = {(v, m) for v, m, _ in (CASES if cases is None else cases)}
    want = expected_pairs()
    missing, extra = sorted(want - have), sorted(have - want)
    assert not missing, "CASES has no row for (variant, mode): %s" % missing
    assert not extra, "CASES has rows the family table does not admit: %s" % extra
    assert sorted(v for vs in FAMILIES.values() for v in vs) == list(range(1, 42)), "FAMILIES must name every variant once"


def case_id(row):
    return "v%d-%s-%s" % row


def resolved(lib, op):
    return int(lib.sat_conv_resolved_variant(C.byref(op)))


def run_named(lib, op, parity=0, stream=None):
    """launch one conv op; an op that names a variant must run THAT kernel (a fall-back is a failure, never a skip)"""
    if op.variant > 0:
        got = resolved(lib, op)
        assert got == op.variant, "the op names variant %d but the launch would run variant %d" % (op.variant, got)
    L.check(lib.sat_run_ops_parity(C.pointer(op), 1, parity, L.stream() if stream is None else stream), "conv variant %d" % op.variant)


class DummyBuffers(dict):
    """distinct, non-null, 16-byte aligned addresses for a host-only op: nothing dereferences them"""

    def __missing__(self, name):
        self[name] = 0x10000 * (len(self) + 1)
        return self[name]


def build_op(lib, variant, mode, geo, buf):
    """the sat_op of one row; buf[name] is the address of: in0, w, out, w_packed, stat_partial, stat_acc, scale1, shift1, in1,
    scale0, shift0, stat_acc1, gamma1, beta1, running_mean1, running_var1, out1 (only the ones the mode uses are asked for)"""
    g = GEOS[geo] if isinstance(geo, str) else geo
    o = L.SatOp()
    o.kind, o.dtype, o.variant = L.OP_CONV, L.SAT_BF16, variant
    o.in0, o.w, o.out = buf["in0"], buf["w"], buf["out"]
    o.N, o.Hin, o.Win, o.Cin, o.Hout, o.Wout, o.Cout = g["N"], g["H"], g["W"], g["Cin"], g["Hout"], g["Wout"], g["Cout"]
    o.KH, o.KW, o.stride, o.pad = g["KH"], g["KW"], g["stride"], g["pad"]
    if g["padw"] != g["pad"]:
        o.flags, o.pad_w = L.CONV_PADW, g["padw"]
    if g["layout"] == "stem":
        o.sN, o.sH, o.sW = g["H"] * g["W"] * 4, g["W"] * 4, 4
    else:
        o.sN, o.sH, o.sW = g["H"] * g["W"] * g["Cin"], g["W"] * g["Cin"], g["Cin"]
    o.ldc = g["ldc"]
    if variant in NEEDS_PACKED:
        o.w_packed = buf["w_packed"]
    stats = mode if mode in STATS else ("atomic" if mode in BN + ADMITS["ay"] else "none")
    if stats == "slab":
        o.stat_partial, o.tiles_m = buf["stat_partial"], lib.sat_conv_tiles_m(g["M"])
    elif stats == "atomic":
        o.stat_acc = buf["stat_acc"]
    if mode in EVAL:
        o.scale1, o.shift1, o.flags = buf["scale1"], buf["shift1"], o.flags | 1
        if mode == "eval_res":
            o.in1 = buf["in1"]
    if mode in ("bn_table", "ay_table"):
        o.scale0, o.shift0 = buf["scale0"], buf["shift0"]
    if mode in ("bn_derive", "ay_derive"):
        o.stat_acc1, o.gamma1, o.beta1 = buf["stat_acc1"], buf["gamma1"], buf["beta1"]
        o.running_mean1, o.running_var1 = buf["running_mean1"], buf["running_var1"]
        o.count, o.momentum, o.eps = g["N"] * g["H"] * g["W"], 0.1, 1e-5
    if mode in ADMITS["ay"]:
        o.in1, o.out1, o.flags = buf["in1"], buf["out1"], o.flags | L.CONV_IN_RESIDUAL
    return o


def host_op(lib, variant, mode, geo):
    return build_op(lib, variant, mode, geo, DummyBuffers())
