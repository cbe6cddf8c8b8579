"""The weight-gradient configuration matrix: one table for tests/test_conv_wgrad_matrix_host.py (which variant does
``ops.conv1d_wgrad_plan`` say a case reaches, and does the table cover every variant) and for
tests/test_conv_wgrad_matrix_gpu.py (does that variant compute the right gradient).

A case = a geometry + the variant it is there for, ``expect``: a partial dict over the keys of
``ops.conv1d_wgrad_plan``, evaluated with ``weight_norm=case.wn, has_bias=True``.  Geometry keys: B, cin, cout, t (input
rows), k, stride, dil, pad (left = right unless ``pad_right``), groups, width, transposed (+ out_pad), slope (None = no
pre-activation, 0.0 = ReLU), wn (weight-normalised: the GPU file runs the ``_wn`` entry point as well), hint (concurrency
hint in force while the case is planned and run).

What the dispatcher can select without environment overrides (tools/sweep_wgrad_plan.py: k 1..41, stride 1..13, dilation
1..512, width 1..40, 128 -> 128 and 32 -> 32 channels, plain and pre-activated):
  * (small, tg): the 32 x 32 tile with tg 1..4 and the 64 x 64 tile with tg 1..7 -- every one is in REQUIRED below; no tg
    is reachable through PWG_WG_TG only;
  * per-tap windows only on the 32 x 32 tile: the 64 x 64 tile's cost loop answers far-apart taps with one tap per
    workgroup ("big_far_taps"), so its WIN instantiations are not reachable without an override (PWG_WG_TG), not covered;
  * 128-column chunks only with a single tap (k = 1): with more, the 32 x 32 tile's buffers pass 80 KiB;
  * dword row staging of MODE 4 (rows_x4 false) only on the 32 x 32 tile: rows that long exceed the LDS on the other;
  * MODE 3 with compile-time stride 3 AND activation is no instantiation (an activated stride-3 layer runs the run-time
    stride loop, "s3_act" pins that), so REQUIRED has (3, plain) only.

Tolerance: every case meets the family's 3e-5 of the largest reference entry against float64 -- the largest error
measured over the whole table is 6.2e-7 -- so no case carries a bar taken from the fp32-ATen error.
"""
import contextlib
import math
import os

# PWG_WG_* (tile, taps, chunk, rows, PWG_WG_K1, ...), PWG_SMALL_CIN, and PWG_CONV_FILL_SCALE, which replaces the concurrency hint
OVERRIDE_PREFIXES = ("PWG_WG_", "PWG_SMALL_CIN", "PWG_CONV_FILL_SCALE")


def overrides_set():
    """Names of the environment overrides that change the weight-gradient plan (the plan assertions skip under them)."""
    return sorted(k for k in os.environ if k.startswith(OVERRIDE_PREFIXES))


def _c(name, expect, B, cin, cout, t, k, stride=1, dil=1, pad=0, groups=1, width=1, transposed=False, out_pad=0,
       slope=None, wn=False, hint=None, pad_right=None):
    return dict(name=name, expect=expect, B=B, cin=cin, cout=cout, t=t, k=k, stride=stride, dil=dil, pad=pad,
                pad_right=pad if pad_right is None else pad_right, groups=groups, width=width, transposed=transposed,
                out_pad=out_pad, slope=slope, wn=wn, hint=hint)


CASES = [
    # ---- 32 x 32 tile: taps split over the four waves --------------------------------------------------------------
    # k = 3 on 4 taps per block: the last wave owns zero taps, k no multiple of taps_block; n_cols = 1 (one column per item)
    _c("small_tg1_idle_wave", dict(path="mfma", small=True, tg=1, taps_block=4, tt=32, mode=0, finisher="direct"),
       B=3, cin=31, cout=33, t=1, k=3, pad=1),
    # k = 7 on 8 taps per block (waves own 2, 2, 2, 1); 64 <= n_cols < 128: 64-column chunks, n_cols = tt + 1
    _c("small_tg2_tt64", dict(small=True, tg=2, taps_block=8, tt=64, mode=1, win=False, act=True),
       B=2, cin=32, cout=63, t=65, k=7, pad=3, slope=0.1),
    # k = 11 on 12 taps (waves own 3, 3, 3, 2); n_cols = tt exactly
    _c("small_tg3_tt64", dict(small=True, tg=3, taps_block=12, tt=64, mode=0, win=False, act=False),
       B=2, cin=65, cout=32, t=64, k=11, pad=5),
    # 128-column chunks keep two workgroups per CU only with a single tap (k = 1); 257 columns are no multiple of 4, so
    # the 1 x 1 kernel of wgrad_k1.hip does not take the layer
    _c("small_tt128_k1", dict(path="mfma", small=True, tg=1, tt=128, mode=1), B=2, cin=32, cout=40, t=257, k=1, slope=0.1),
    # k = 41: three tap groups of 16, the last holds 9 taps (waves own 4, 4, 1, 0); groups with ragged channel counts
    _c("small_tg4_groups", dict(small=True, tg=4, taps_block=16, tap_groups=3, tt=64),
       B=2, cin=80, cout=48, t=300, k=41, pad=20, groups=2, slope=0.2),
    # n_cols below tt = 32
    _c("small_tt32_short", dict(small=True, tt=32, mode=0), B=2, cin=24, cout=31, t=19, k=5, pad=2),
    # ---- 64 x 64 tile: every tg of the cost loop ----------------------------------------------------------------------
    _c("big_tg1", dict(small=False, tg=1, tt=32, mode=0, win=False), B=2, cin=33, cout=65, t=33, k=1),
    _c("big_tg2", dict(small=False, tg=2, mode=1), B=2, cin=64, cout=64, t=32, k=2, pad=1, slope=0.1),
    _c("big_tg3", dict(small=False, tg=3, tap_groups=1, mode=0), B=2, cin=63, cout=65, t=31, k=3, pad=1),
    _c("big_tg4", dict(small=False, tg=4), B=1, cin=65, cout=63, t=70, k=4, pad=2),
    _c("big_tg5", dict(small=False, tg=5), B=2, cin=40, cout=72, t=50, k=5, pad=2, slope=0.0),
    _c("big_tg6_s8", dict(small=False, tg=6, mode=3, stride_ct=8, act=False), B=2, cin=40, cout=40, t=203, k=6, stride=8, pad=2),
    _c("big_tg7", dict(small=False, tg=7, tap_groups=1), B=2, cin=48, cout=34, t=90, k=7, pad=3),
    # k = 11 in 4 groups of 3: the last group holds 2 taps
    _c("big_tg3_ragged_groups", dict(small=False, tg=3, tap_groups=4), B=2, cin=34, cout=34, t=100, k=11, dil=3, pad=15, slope=0.1),
    # groups > 1 with 40 in / 72 out per group on the 64 x 64 tile
    _c("big_groups_ragged", dict(small=False, tiles=6), B=2, cin=120, cout=216, t=64, k=3, pad=1, groups=3),
    # ---- per-tap windows (stride 1, width 1, (ntaps - 1) * dil > 96) ----------------------------------------------------
    # (32 x 32 tile only: on the 64 x 64 tile the cost model answers far-apart taps with one tap per workgroup, see
    # "big_far_taps"; its WIN instantiations need PWG_WG_TG -- not reachable without an override, not covered)
    _c("win_mode0", dict(win=True, small=True, mode=0, act=False), B=2, cin=32, cout=40, t=400, k=3, dil=64, pad=64),
    _c("win_mode1", dict(win=True, small=True, mode=1, act=True), B=2, cin=40, cout=31, t=300, k=3, dil=128, pad=128,
       slope=0.2),
    _c("win_dil512", dict(win=True, small=True, mode=1, tt=64), B=1, cin=32, cout=32, t=1100, k=3, dil=512, pad=512, slope=0.1),
    # the threshold: (3 - 1) * 48 = 96 shares one tile, (2 - 1) * 97 = 97 takes the windows
    _c("win_threshold_96", dict(win=False, small=True, mode=0), B=2, cin=32, cout=40, t=200, k=3, dil=48, pad=48),
    _c("win_threshold_97", dict(win=True, small=True, mode=0), B=2, cin=32, cout=40, t=200, k=2, dil=97, pad=48, pad_right=49),
    _c("big_far_taps", dict(win=False, small=False, tg=1, tap_groups=3, mode=1), B=2, cin=40, cout=40, t=300, k=3, dil=128,
       pad=128, slope=0.1),
    # ---- MODE 3: strided, width 1 ----------------------------------------------------------------------------------
    _c("s2", dict(mode=3, stride_ct=2, act=False), B=2, cin=40, cout=40, t=130, k=4, stride=2, pad=1),
    _c("s2_act", dict(mode=3, stride_ct=2, act=True), B=2, cin=24, cout=40, t=131, k=5, stride=2, pad=2, slope=0.1),
    _c("s3", dict(mode=3, stride_ct=3, act=False), B=2, cin=8, cout=24, t=50, k=5, stride=3, pad=2),
    # (there is no activated compile-time stride 3: the run-time loop)
    _c("s3_act", dict(mode=3, stride_ct=0, act=True), B=2, cin=40, cout=33, t=100, k=5, stride=3, pad=2, slope=0.1),
    _c("s4", dict(mode=3, stride_ct=4, act=False), B=2, cin=36, cout=36, t=257, k=9, stride=4, pad=4),
    _c("s4_act_groups", dict(mode=3, stride_ct=4, act=True, small=True, tg=4), B=2, cin=64, cout=128, t=400, k=41, stride=4,
       pad=20, groups=2, slope=0.2),
    _c("s8_act", dict(mode=3, stride_ct=8, act=True), B=2, cin=40, cout=40, t=260, k=16, stride=8, pad=4, slope=0.1),
    _c("s5", dict(mode=3, stride_ct=0, act=False), B=2, cin=40, cout=40, t=161, k=10, stride=5, pad=3),
    _c("s11_act", dict(mode=3, stride_ct=0, act=True), B=2, cin=33, cout=40, t=230, k=5, stride=11, pad=2, slope=0.0),
    # ConvTranspose1d: x is the G operand (the activation slope lands on it), dy the strided one; bias by bias_grad_kernel
    _c("convt_s8_act", dict(mode=3, stride_ct=8, act=True), B=2, cin=64, cout=40, t=32, k=16, stride=8, pad=4, transposed=True,
       slope=0.1),
    _c("convt_s5", dict(mode=3, stride_ct=0, act=False), B=1, cin=40, cout=36, t=28, k=10, stride=5, pad=3, out_pad=1,
       transposed=True),
    # StyleMelGAN's noise upsampler (CONVT_CASES of test_conv_ops_gpu.py): the X rows of a 64 x 64 tile exceed the LDS even
    # with one tap per workgroup, the plan's second pass drops to the 32 x 32 tile
    _c("convt_s11_second_pass", dict(small=True, mode=3, stride_ct=0, act=True), B=4, cin=128, cout=64, t=1, k=22, stride=11,
       pad=6, out_pad=1, transposed=True, slope=0.2),
    # ---- MODE 2: (k,1) with width > 32 (per-lane row wrap) ------------------------------------------------------------
    _c("w37", dict(mode=2, act=False, rows_half=0), B=2, cin=24, cout=40, t=20, k=5, stride=3, pad=2, width=37),
    _c("w37_act", dict(mode=2, act=True, rows_half=0), B=2, cin=40, cout=33, t=23, k=5, stride=3, pad=2, width=37, slope=0.1),
    _c("w34", dict(mode=2, act=False, rows_half=0), B=1, cin=40, cout=40, t=17, k=3, stride=2, pad=1, width=34),
    _c("w34_act", dict(mode=2, act=True, rows_half=0, small=True), B=2, cin=16, cout=40, t=30, k=5, stride=4, pad=2, width=34,
       slope=0.2),
    # width <= 32, but one strided row pair of 257 floats leaves no rows_half that fits the LDS: MODE 2 on the 64 x 64 tile
    _c("w32_no_rows", dict(mode=2, act=False, rows_half=0, small=False), B=1, cin=40, cout=40, t=64, k=1, stride=7, width=32),
    # ---- MODE 4: (k,1) with row-aligned chunks -----------------------------------------------------------------------
    # odd width, h_out = 34 no multiple of 2 * rows_half, window start -2 * 3 = -6: negative and no multiple of 4
    _c("rows_w3_x4", dict(mode=4, rows_x4=True, act=True), B=2, cin=32, cout=128, t=100, k=5, stride=3, pad=2, width=3,
       slope=0.1),
    _c("rows_w2_x4_big", dict(mode=4, rows_x4=True, act=False, small=False), B=2, cin=40, cout=40, t=67, k=5, stride=3, pad=2,
       width=2),
    _c("rows_w5_x4_unaligned", dict(mode=4, rows_x4=True), B=2, cin=33, cout=40, t=45, k=5, stride=3, pad=1, width=5, slope=0.1),
    _c("rows_w11", dict(mode=4, rows_x4=True, act=True), B=2, cin=16, cout=16, t=9, k=5, stride=3, pad=2, width=11, slope=0.1),
    # rows of (4 + 4 + 1) * 29 = 261 floats are too long for one 16-byte DMA instruction per row: dword pieces (32 x 32 tile
    # only: on the 64 x 64 tile such rows exceed the LDS and the layer stays in MODE 2)
    _c("rows_w29_dword", dict(mode=4, rows_x4=False, act=True, rows_half=1), B=2, cin=16, cout=40, t=30, k=5, stride=4, pad=2,
       width=29, slope=0.1),
    _c("rows_w32_dword", dict(mode=4, rows_x4=False, act=False, rows_half=1), B=2, cin=40, cout=16, t=21, k=5, stride=3, pad=2,
       width=32),
    # 40 -> 40 channels, but the strided rows of width 30 exceed the LDS on the 64 x 64 tile: the plan's second pass
    _c("rows_w30_second_pass", dict(mode=4, rows_x4=False, small=True, tiles=4), B=1, cin=40, cout=40, t=25, k=5, stride=4,
       pad=2, width=30),
    # ---- finishers --------------------------------------------------------------------------------------------------
    _c("fin_slabs", dict(path="mfma", finisher="slabs"), B=3, cin=40, cout=40, t=700, k=3, pad=1),
    _c("fin_slabs_wide", dict(path="mfma", finisher="slabs_wide"), B=4, cin=40, cout=40, t=1100, k=3, pad=1, slope=0.1),
    # weight norm: splits >= 16 under n0 < 512 -> wide slab sum + pwg_weight_norm_backward
    _c("wn_two_kernel", dict(path="mfma", finisher="wn_two_kernel"), B=2, cin=64, cout=64, t=2048, k=3, pad=1, wn=True),
    # n0 >= 512, splits >= 16, rows of 120 floats: the 8-slab-lane fused finisher; 2 x 2048 columns
    _c("wn_fused_wide", dict(path="mfma", finisher="wn_fused_wide"), B=2, cin=40, cout=512, t=2048, k=3, pad=1, wn=True,
       slope=0.1),
    # a row of 1920 floats: 9 x 7680 B exceeds the wide form's 64 KiB
    _c("wn_fused_long_row", dict(path="mfma", finisher="wn_fused"), B=2, cin=640, cout=40, t=40, k=3, pad=1, wn=True),
    # n0 = 300: two bias workgroups behind the rows, the second one ragged; one slice (the slab still goes through the finisher)
    _c("wn_fused_bias_ragged", dict(path="mfma", finisher="wn_fused"), B=2, cin=33, cout=300, t=50, k=3, pad=1, wn=True,
       slope=0.1),
    _c("wn_rows_mode4", dict(mode=4, finisher="wn_fused"), B=2, cin=32, cout=40, t=61, k=5, stride=3, pad=2, width=3, wn=True,
       slope=0.1),
    _c("wn_convt", dict(mode=3, finisher="wn_fused"), B=2, cin=64, cout=33, t=40, k=4, stride=2, pad=1, transposed=True, wn=True,
       slope=0.1),
    # ---- slices and padding -----------------------------------------------------------------------------------------
    # 3 items x 11 chunks in slices that end inside an item, the last one shorter
    _c("slices_ragged", dict(path="mfma", finisher="slabs"), B=3, cin=40, cout=40, t=340, k=3, pad=1),
    # left padding of more than a 32-column chunk; left-only (causal) padding; none
    _c("pad_gt_chunk", dict(mode=0, tt=32), B=2, cin=40, cout=40, t=100, k=5, dil=10, pad=40),
    _c("pad_causal", dict(mode=1), B=2, cin=40, cout=40, t=90, k=3, dil=4, pad=8, pad_right=0, slope=0.1),
    _c("pad_zero", dict(mode=0), B=2, cin=40, cout=40, t=90, k=3),
    # fewer resident workgroups under a concurrency hint: 512 / 2 tiles instead of 768 / 2
    _c("hint_below_1", dict(path="mfma", finisher="slabs_wide"), B=8, cin=40, cout=72, t=16384, k=3, pad=1, hint=0.5),
    # ---- the router: one case per path that is not conv1d_wgrad_kernel -----------------------------------------------
    _c("path_gconv", dict(path="gconv", finisher="slabs"), B=2, cin=16, cout=64, t=400, k=41, stride=4, pad=20, groups=4,
       slope=0.2),
    _c("path_small_cin", dict(path="small_cin"), B=2, cin=1, cout=16, t=2100, k=15, pad=7),
    _c("path_k1", dict(path="k1"), B=8, cin=48, cout=48, t=4096, k=1, wn=True),
]

BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def out_rows(c):
    """Output rows per item (t_out of the descriptor)."""
    if c["transposed"]:
        return (c["t"] - 1) * c["stride"] - 2 * c["pad"] + c["k"] + c["out_pad"]
    return (c["t"] + c["pad"] + c["pad_right"] - c["dil"] * (c["k"] - 1) - 1) // c["stride"] + 1


def make_desc(c):
    from parallelwavegan_amd import ops

    pre = None if c["slope"] is None else ("relu" if c["slope"] == 0.0 else "leaky_relu")
    return ops.make_conv_desc(c["B"], c["cin"], c["cout"], c["t"], out_rows(c), c["k"], c["stride"], c["dil"], c["pad"],
                              c["groups"], transposed=c["transposed"], width=c["width"], pre_act=pre,
                              pre_slope=c["slope"] or 0.0)


@contextlib.contextmanager
def concurrency_hint(value):
    """The case's concurrency hint (None: leave it alone), restored afterwards."""
    if value is None:
        yield
        return
    from parallelwavegan_amd import _lib

    was = _lib.lib().pwg_set_concurrency_hint(value)
    try:
        yield
    finally:
        _lib.lib().pwg_set_concurrency_hint(was)


def plan_of(c, weight_norm=None, has_bias=True):
    from parallelwavegan_amd import ops

    with concurrency_hint(c["hint"]):
        return ops.conv1d_wgrad_plan(make_desc(c), weight_norm=c["wn"] if weight_norm is None else weight_norm,
                                     has_bias=has_bias)


def roles(c):
    """(co_g, ci_g, n_cols, x_len) in the kernel's roles: G operand rows, X operand rows, reduction columns per item."""
    g = c["groups"]
    if c["transposed"]:
        return c["cin"] // g, c["cout"] // g, c["t"] * c["width"], out_rows(c) * c["width"]
    return c["cout"] // g, c["cin"] // g, out_rows(c) * c["width"], c["t"] * c["width"]


def covered(c, p):
    """The coverage items case ``c`` contributes under plan ``p`` -- computed from the plan and the geometry, never from
    the case's name or its ``expect``."""
    items = {("path", p["path"]), ("finisher", p["finisher"])}
    co_g, ci_g, n_cols, _ = roles(c)
    # the fused weight-norm finisher's bias workgroups (256 rows each) behind its n0 row workgroups: more than one, the
    # last one ragged; a transposed layer's bias comes from bias_grad_kernel, its finisher has none
    n0 = co_g * c["groups"]
    if c["wn"] and not c["transposed"] and n0 > 256 and n0 % 256 and p["finisher"] in ("wn_fused", "wn_fused_wide"):
        items.add(("wn_bias_rows_ragged",))
    if p["path"] != "mfma":
        return items
    k, W, mode = c["k"], c["width"], p["mode"]
    items.add(("tile", p["small"], p["tg"]))
    if p["small"]:
        if mode != 4:
            items.add(("small_tt", p["tt"]))
        # a block with at most 3 * tg taps leaves the last wave none
        if any(min(p["taps_block"], k - b * p["taps_block"]) <= 3 * p["tg"] for b in range(p["tap_groups"])):
            items.add(("small_idle_wave",))
        if k % p["taps_block"]:
            items.add(("small_ragged_taps",))
    elif k % p["tg"]:
        items.add(("big_ragged_taps",))
    if mode in (0, 1):
        items.add(("win", p["win"], mode))
        flat_dil = c["dil"] * W  # (a stride-1 (k,1) layer runs flattened)
        span = (min(k, p["taps_block"]) - 1) * flat_dil
        if span in (96, 97):
            items.add(("win_threshold", span))
    if mode == 3:
        items.add(("mode3", p["stride_ct"], p["act"]))
        if c["transposed"] and p["act"]:
            items.add(("mode3_slope_on_g",))
        if c["transposed"] and p["small"] and co_g > 32 and ci_g > 32:
            items.add(("second_pass_small",))
    if mode == 2:
        items.add(("mode2", p["act"], "odd" if W % 2 else "even"))
    if mode == 4:
        items.add(("mode4", p["rows_x4"]))
        h_out = n_cols // W
        if W % 2:
            items.add(("mode4_odd_width",))
        if h_out % (2 * p["rows_half"]):
            items.add(("mode4_ragged_rows",))
        if p["rows_x4"]:
            # X window starts f0 of every (chunk, tap group), as the kernel's issue() computes them: a start that is no
            # multiple of 4 is moved down (sh = f0 & 3), a negative one begins in the top padding; fix_tail stores
            # exactly when the 16-byte piece at the end of a row straddles it (its own condition on es)
            x_len = c["t"] * W
            starts = [(h0 * c["stride"] + z * p["taps_block"] * c["dil"] - c["pad"]) * W
                      for h0 in range(0, h_out, 2 * p["rows_half"]) for z in range(p["tap_groups"])]
            if any(f % 4 for f in starts):
                items.add(("mode4_x4_realign",))
            if any(f < 0 for f in starts):
                items.add(("mode4_x4_negative_start",))
            ends = [x_len - (f & ~3) for f in starts]
            if x_len % 4 and any(0 < es < p["xs_stride"] - 4 and es % 4 for es in ends):
                items.add(("mode4_x4_tail_repair",))
    # tile edges
    for what, v in (("co_g", co_g), ("ci_g", ci_g)):
        if v in (31, 32, 33, 63, 64, 65):
            items.add((what, v))
    bt = 32 if p["small"] else 64
    if c["groups"] > 1 and co_g % bt and ci_g % bt:
        items.add(("groups_ragged", p["small"]))
    chunk = 2 * p["rows_half"] * W if mode == 4 else p["tt"]
    if n_cols == 1:
        items.add(("n_cols", "one"))
    elif n_cols < chunk:
        items.add(("n_cols", "below_chunk"))
    elif n_cols == chunk:
        items.add(("n_cols", "chunk"))
    elif n_cols == chunk + 1:
        items.add(("n_cols", "chunk_plus_1"))
    per_item = math.ceil(n_cols / chunk)
    total = per_item * c["B"]
    per_block = math.ceil(total / p["splits"])
    if p["splits"] > 1 and total % per_block:
        items.add(("last_slice_short",))
    if any((s * per_block) % per_item for s in range(1, p["splits"])):
        items.add(("slice_inside_item",))
    if mode != 4 and W == 1:
        if c["pad"] > chunk:
            items.add(("pad", "left_gt_chunk"))
        if c["pad"] > 0 and c["pad_right"] == 0:
            items.add(("pad", "causal"))
        if c["pad"] == 0 and c["pad_right"] == 0 and k > 1:
            items.add(("pad", "zero"))
    if c["hint"] is not None and c["hint"] < 1.0:
        items.add(("hint_below_1",))
    return items


REQUIRED = (
    {("tile", True, tg) for tg in (1, 2, 3, 4)} | {("tile", False, tg) for tg in (1, 2, 3, 4, 5, 6, 7)}
    | {("small_idle_wave",), ("small_ragged_taps",), ("big_ragged_taps",)}
    | {("small_tt", tt) for tt in (32, 64, 128)}
    | {("win", win, mode) for win in (True, False) for mode in (0, 1)}
    | {("win_threshold", 96), ("win_threshold", 97)}
    | {("mode3", s, act) for s in (0, 2, 4, 8) for act in (True, False)} | {("mode3", 3, False)}
    | {("mode3_slope_on_g",), ("second_pass_small",)}
    | {("mode2", act, par) for act in (True, False) for par in ("odd", "even")}
    | {("mode4", True), ("mode4", False), ("mode4_odd_width",), ("mode4_ragged_rows",), ("mode4_x4_realign",),
       ("mode4_x4_negative_start",), ("mode4_x4_tail_repair",)}
    | {("finisher", f) for f in ("direct", "slabs", "slabs_wide", "wn_two_kernel", "wn_fused", "wn_fused_wide")}
    | {("wn_bias_rows_ragged",)}
    | {("path", p) for p in ("mfma", "gconv", "small_cin", "k1")}
    | {(what, v) for what in ("co_g", "ci_g") for v in (31, 32, 33, 63, 64, 65)}
    | {("groups_ragged", True), ("groups_ragged", False)}
    | {("n_cols", v) for v in ("one", "below_chunk", "chunk", "chunk_plus_1")}
    | {("last_slice_short",), ("slice_inside_item",)}
    | {("pad", v) for v in ("left_gt_chunk", "causal", "zero")}
    | {("hint_below_1",)}
)
