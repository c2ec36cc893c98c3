// The chunk-column launch geometry of the element-wise kernels (norm_act.hip, elementwise.hip, the heads of head_loss.hip):
// 256 threads per block, one thread column per 8-channel chunk, CT columns x PY pixel rows.
#pragma once
#include "common.h"

// (internal linkage, and EwShape stays the anonymous-namespace type the kernels' mangled names carry)
namespace {

constexpr int NTHR = 256;

struct EwShape {
    int N, H, W, Cp;
    int CPP;  // 8-channel chunks per pixel
    int CT;   // chunk columns per block (power of two <= 32)
    int PY;   // pixel rows per block = 256 / CT
};

static EwShape make_shape(int N, int H, int W, int Cp) {
    EwShape s;
    s.N = N; s.H = H; s.W = W; s.Cp = Cp;
    s.CPP = Cp / 8;
    int ct = 1;
    while (ct < s.CPP && ct < 32) ct <<= 1;
    s.CT = ct;
    s.PY = NTHR / ct;
    return s;
}

// one item per thread row: block columns over the chunk tiles, at most max_blocks blocks in all
static dim3 make_grid_dense(const EwShape& s, long long items, int max_blocks) {
    const int gy = ceil_div(s.CPP, s.CT);
    long long gx = (items + s.PY - 1) / s.PY;
    long long cap = max_blocks / gy;
    if (cap < 1) cap = 1;
    if (gx > cap) gx = cap;
    if (gx < 1) gx = 1;
    return dim3((unsigned)gx, (unsigned)gy);
}

static dim3 make_grid(const EwShape& s, long long items, int max_blocks = 2048) {
    // few, fat blocks: every block ends with one atomic per channel into the same addresses, and
    // same-address atomics serialise (MI355X_MICROARCH: ~14x slower than spread ones)
    dim3 grid = make_grid_dense(s, items, max_blocks);
    const long long want = (items + 4ll * s.PY - 1) / (4ll * s.PY);     // >= 4 items per thread
    if (grid.x > want) grid.x = want < 1 ? 1u : (unsigned)want;
    return grid;
}

// items of a pass over [N][H][W]: pixels, or -- 2x2 windows (pooling forward, pooled gradient backward) -- one item per pixel
// column of a row pair, over an even padded width
static long long walk_items(int N, int H, int W, bool windows) {
    return windows ? (long long)N * ((H + 1) / 2) * (2 * ((W + 1) / 2)) : (long long)N * H * W;
}

int check_ew(int N, int H, int W, int Cp) {
    SEGNB_CHECK_ARG(N > 0 && H > 0 && W > 0 && Cp > 0 && Cp % 8 == 0, "bad NHWC shape (Cp % 8 != 0?)");
    SEGNB_CHECK_ARG((long long)N * H * W * 4 < (1ll << 31), "pixel count exceeds int32");
    return 0;
}

// exact a / d for 0 <= a < 2^31 through a double reciprocal (8 instructions; the integer division sequence is ~35 and
// the pooled kernels are VALU-bound): the truncated product is off by at most one, the remainder says which way
struct FastDiv {
    int d;
    double inv;
    __device__ __forceinline__ explicit FastDiv(int d_) : d(d_), inv(1.0 / (double)d_) {}
    __device__ __forceinline__ int div(int a) const {
        const int q = (int)((double)a * inv);
        const int r = a - q * d;
        return q + (r >= d ? 1 : 0) - (r < 0 ? 1 : 0);
    }
};

}  // namespace
