// vt_window_index.h -- the index maps of shifted-window attention (reference backbones/swin.py:16-86) as pure integer
// functions, shared by the kernels of vt_window_attention.hip and by host programs (a plain C++ compiler takes this file).
//
// All coordinates are UN-ROLLED pixel coordinates of the [H][W] map; the reference's roll(-shift) -> window_partition ->
// attention -> window_unpartition -> roll(+shift) is the statement that token t = i ws + j of window (wy, wx) IS pixel
// ((wy ws + i + shift) mod H, (wx ws + j + shift) mod W), for the loads and for the store.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VT_WIN_FN __host__ __device__ inline
#else
#define VT_WIN_FN inline
#endif

// pixel (y, x) of token t of window (wy, wx)
VT_WIN_FN void vt_win_pixel(int wy, int wx, int t, int ws, int shift, int H, int W, int* y, int* x) {
    const int i = t / ws, j = t - i * ws;
    *y = (wy * ws + i + shift) % H;
    *x = (wx * ws + j + shift) % W;
}

// region of the ROLLED coordinate c = w ws + i along an axis of n pixels (swin.py:51: the slices 0:-ws, -ws:-shift, -shift:);
// two tokens of a window may attend to each other only where their regions agree along both axes.  shift = 0: one region.
VT_WIN_FN int vt_win_region(int c, int n, int ws, int shift) {
    if (shift <= 0) return 0;
    return c < n - ws ? 0 : (c < n - shift ? 1 : 2);
}

// 3 r_y + r_x of token t of window (wy, wx): the value the reference's img_mask holds at that token
VT_WIN_FN int vt_win_token_region(int wy, int wx, int t, int ws, int shift, int H, int W) {
    const int i = t / ws, j = t - i * ws;
    return 3 * vt_win_region(wy * ws + i, H, ws, shift) + vt_win_region(wx * ws + j, W, ws, shift);
}

// index into a head's (2 ws - 1)^2 relative-position table for query token (iq, jq) and key token (ik, jk)
VT_WIN_FN int vt_win_rel_index(int iq, int jq, int ik, int jk, int ws) {
    return (iq - ik + ws - 1) * (2 * ws - 1) + (jq - jk + ws - 1);
}
