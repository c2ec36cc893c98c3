// Which instantiation of conv_fprop_ws_kernel (fprop_dma.hip) and of conv_fprop_rw_kernel (fprop_rw.hip) serves a launch: the
// configuration tables of the two files and the one rule that picks a row, a form and a store-row order from the facts of a launch
// and the values of the knobs.  Plain C++17 with no HIP in it, no knob call and no allocation: the launchers build the facts, read the
// knobs and call ws_select / rw_select once per launch; the predicates ask the same functions; the host test
// (tests/test_ws_tile14_cpu.py) compiles this file with the host compiler alone and compares it with the rule it replaced.
#pragma once

// ---- conv_fprop_ws_kernel -------------------------------------------------------------------------------------------------------
// rows of WS_TILES, in table order; the first four are the values of segnb_tune "fprop_dma_cfg"
enum { WS_8x32, WS_16x16, WS_TALL, WS_14x14, WS_UPD_8x32, WS_UPD_16x16, WS_UPF_8x32, WS_UPF_16x16, WS_NROWS, WS_NONE = -1 };
// instantiation forms <DBG, EP, STATS, SPLITK, MASK> of a row: statistics (the plain form), none, activation mask, affine epilogue,
// timing build, split K with and without statistics
enum { WS_STATS, WS_NOSTATS, WS_MASK, WS_EP, WS_DBG, WS_KS_STATS, WS_KS_NOSTATS, WS_NFORMS };
// the window of a launch: 3 x 3, the plane gather (data gradient of an up-sampled segment), the phase forward of such a segment
enum { WS_WIN_3x3, WS_WIN_UPD, WS_WIN_UPF };

struct WsTile {
    int BN, R, WT, CW_M;
    bool TALL, MF16;
    int NTAP, UP;
    int BM;                 // matrix rows of a tile (WsCfg::BM)
    unsigned forms;         // bit f: the row has form f in the plain order of the store rows ...
    unsigned epi_forms;     // ... and on peeled, straight-line taps (WsEpi)
    const char* tag;        // call census: which row served a launch
};
constexpr unsigned ws_bits() { return 0u; }
template <class... F>
constexpr unsigned ws_bits(int f, F... more) { return (1u << f) | ws_bits(more...); }

// 8 x 32 and 16 x 16 pixels in 256 rows; 7 x 7 images as one tall image in tiles of 36 x 7 (odd halo pitch: the 32x32x16 stream; its
// split K); 14 x 14 pixels in 224 rows (statistics / none only); the two tiles of the plane gather (no statistics, no epilogue) and of
// the phase forward (statistics of the sums).  The WsEpi order exists for the 16x16x32 forms of the 3 x 3 window that the ZF_UNET step
// launches without split K, never with the affine epilogue.
static constexpr WsTile WS_TILES[WS_NROWS] = {
    {64, 8, 32, 4, false, true, 9, 0, 256, ws_bits(WS_STATS, WS_NOSTATS, WS_EP, WS_DBG), 0u, "tile:ws8x32"},
    {64, 16, 16, 4, false, true, 9, 0, 256, ws_bits(WS_STATS, WS_NOSTATS, WS_MASK, WS_EP, WS_DBG),
     ws_bits(WS_STATS, WS_NOSTATS, WS_MASK, WS_DBG), "tile:ws16"},
    {64, 36, 7, 4, true, false, 9, 0, 256, ws_bits(WS_STATS, WS_NOSTATS, WS_EP, WS_DBG, WS_KS_STATS, WS_KS_NOSTATS), 0u, "tile:wstall"},
    {64, 14, 14, 2, false, true, 9, 0, 224, ws_bits(WS_STATS, WS_NOSTATS), ws_bits(WS_STATS, WS_NOSTATS), "tile:ws14"},
    {64, 8, 32, 4, false, true, 4, 1, 256, ws_bits(WS_NOSTATS), 0u, "tile:ws_upd8x32"},
    {64, 16, 16, 4, false, true, 4, 1, 256, ws_bits(WS_NOSTATS), 0u, "tile:ws_upd16"},
    {64, 8, 32, 4, false, true, 4, 2, 256, ws_bits(WS_STATS), 0u, "tile:ws_upf8x32"},
    {64, 16, 16, 4, false, true, 4, 2, 256, ws_bits(WS_STATS), 0u, "tile:ws_upf16"},
};

// The levels at which the 14 x 14 tile is the default (bit k: square images of 14 << k pixels): measured per launch of the bs = 32
// 224 x 224 step (tools/tile14_bench.py, profiles/tile14_ab.txt) -- forced, all 18 launches at 56^2, 28^2 and 14^2
// are 6-12 % faster; by default it serves the 12 whose every stored bit AND statistic stays the 16 x 16 tile's (ws_select:
// same_stats), 741 -> 700 us in sum.  Other sizes made of 14 x 14 tiles (42^2, 28 x 56 ...) take the tile under the knob only.
constexpr unsigned WS14_DEFAULT_LEVELS = 7u;

struct WsFacts {
    int N, H, W;            // output grid
    int Hi, Wi, Ci, Co;
    bool stats, mask, ep, upcat, dbg;      // statistics (the mask's sums among them) / activation mask / affine epilogue / virtual concat / timing build
    bool row_major;         // the taps are in row-major order (either direction): the 16x16x32 form indexes its address tables by (t / 3, t % 3)
    int window;             // WS_WIN_*
    bool no_prev;           // phase forward: nothing to accumulate into
    bool bias;              // a bias vector comes with the launch (the plane gather takes none)
};
struct WsKnobs {
    bool dma, upd, mask;    // segnb_tune "fprop_dma", "fprop_upd", "fprop_mask"
    int cfg, epi, ksplit, nostats;      // "fprop_dma_cfg", "fprop_dma_epi", "fprop_ksplit", "fprop_nostats"
    int cus;                // CUs a launch may use ("conv_cu_pct")
    unsigned levels14;      // WS14_DEFAULT_LEVELS
};
struct WsChoice {
    int row;                // WS_TILES row or WS_NONE: declined
    int form;               // WS_* form of the launch
    bool epi;               // store rows on straight-line taps (WsEpi)
    int ks;                 // split-K slices wanted (1: none) and the form they launch where the workspace is there
    int ks_form;
};

// persistent blocks per channel tile: the CUs a launch may use over its ntl channel tiles
static inline int ws_blocks(int cus, int ntl) {
    const int gm = cus / ntl;
    return gm < 1 ? 1 : gm;
}
// rounds of (equal) R x WT tiles on gm persistent blocks
static inline long long ws_rounds(int N, int H, int W, int R, int WT, int gm) {
    const long long it = (long long)N * ((H + R - 1) / R) * ((W + WT - 1) / WT);
    return (it + gm - 1) / gm;
}
// 8 x 32 or 16 x 16 pixel tiles: whichever needs fewer rounds of (equal) tiles on the persistent blocks (128 -> 384 @56x56: 11 vs 12
// rounds, 104 vs 122 us; 64 -> 192 @112x112: 21 vs 19 rounds, 133 vs 116 us); ties go to 16 x 16.  *r: the rounds of the tile chosen
static inline int ws_flat_tile(int N, int H, int W, int gm, long long* r = nullptr) {
    const long long r0 = ws_rounds(N, H, W, 8, 32, gm), r1 = ws_rounds(N, H, W, 16, 16, gm);
    if (r != nullptr) *r = r0 < r1 ? r0 : r1;
    return r0 < r1 ? WS_8x32 : WS_16x16;
}

// split K pays where a launch has fewer (pixel tile, channel tile) pairs than half the CUs it may use: the 7 x 7 level of
// lib/models/zf_unet.py:44-56 (8 tall row tiles x 8..16 channel tiles at bs = 32).  Returns the number of slices (1 = no split)
static inline int ws_ksplit(const WsFacts& f, const WsKnobs& k, const WsTile& t) {
    if (!t.TALL || !k.ksplit || f.ep || f.dbg) return 1;
    const long long tiles = (long long)((f.N * (f.H + 1) + t.R - 1) / t.R) * ((f.Co + t.BN - 1) / t.BN);
    const int nch = f.Ci / 64;
    // A data gradient (no statistics) of a two-stream backward runs beside the weight-gradient stream, which sizes its launches
    // for a share of the CUs (wgrad_s1.hip: s1_slabs): slices beyond the CUs that are left would queue behind their partners
    const int cus = f.stats ? k.cus : k.cus / 2;
    int ks = 1;
    if (tiles * 2 <= cus && nch % 2 == 0 && nch / 2 >= 2) ks = 2;
    if (tiles * 4 <= cus && nch % 4 == 0 && nch / 4 >= 2) ks = 4;
    if ((k.ksplit == 2 || k.ksplit == 4) && nch % k.ksplit == 0 && nch / k.ksplit >= 2) ks = k.ksplit;
    if (tiles * ks * 65536ll >= (1ll << 31)) return 1;      // (the slabs behind one buffer descriptor)
    return ks;
}

static inline WsChoice ws_select(const WsFacts& f, const WsKnobs& k) {
    WsChoice c = {WS_NONE, WS_STATS, false, 1, WS_KS_STATS};
    if (!k.dma) return c;
    int row;
    if (f.window == WS_WIN_UPD) {
        // ntaps 16, in_step 2 on the low-resolution grid; planes of 32 channels or of whole 64-channel chunks
        if (!k.upd || !f.row_major || f.stats || f.ep || f.mask || f.bias || f.upcat || f.Hi != 2 * f.H || f.Wi != 2 * f.W) return c;
        if ((f.Ci % 64 != 0 && f.Ci != 32) || f.Co <= 32 || f.W < 12) return c;
        const int flat = k.cfg < 0 ? ws_flat_tile(f.N, f.H, f.W, ws_blocks(k.cus, (f.Co + 63) / 64)) : k.cfg;
        row = flat == WS_8x32 ? WS_UPD_8x32 : WS_UPD_16x16;
        c.form = WS_NOSTATS;
    } else if (f.window == WS_WIN_UPF) {
        if (!k.upd || f.Ci % 64 != 0 || f.Ci < 128 || (f.Co <= 32 && !f.no_prev) || f.W < 12) return c;
        const int flat = k.cfg < 0 ? ws_flat_tile(f.N, f.H, f.W, ws_blocks(k.cus, 4 * ((f.Co + 63) / 64))) : k.cfg;
        row = flat == WS_8x32 ? WS_UPF_8x32 : WS_UPF_16x16;
        c.form = WS_STATS;      // (the activation of segnb_upconv_fprop is applied in this form's staging, not by the EP one)
    } else {
        // A 3 x 3 window in another tap order is declined, as a dilated one is: fprop_s1.hip takes any order through its dh / dw tables
        if (f.Ci % 64 != 0 || !f.row_major) return c;
        if (f.mask && (f.ep || f.upcat || !k.mask)) return c;
        if (f.upcat && f.W <= 8) return c;
        // 14 x 14 tiles serve images whose sides are multiples of 14, with statistics or without, nothing else
        const bool can14 = f.H % 14 == 0 && f.W % 14 == 0 && f.W <= 56 && f.Co > 32 && !f.mask && !f.ep && !f.dbg;
        // "fprop_dma_cfg" forces a row (0: 8 x 32, 1: 16 x 16, 2: tall 36 x 7, 3: 14 x 14 -- a launch the 14 x 14 form does not serve
        // takes its default tile: declined, not refused)
        row = k.cfg == WS_14x14 && !can14 ? -1 : k.cfg;
        if (row < 0) {
            // measured per ZF_UNET layer at bs=32 (tools/layer_bench.py --cfg): 64-channel output tiles win on every level from
            // 14x14 to 112x112.  Outputs of <= 32 channels (half of every tile padding) stay with fprop_s1 / the general kernel.
            if (f.Co <= 32) return c;
            if (f.W <= 8) {
                // 7 x 7 images (the deepest ZF_UNET level): tall-image tiles of 36 x 7 virtual pixels (76 -> ~45 us for 1024 -> 1024)
                if (f.W != 7 || f.H != 7) return c;
                row = WS_TALL;
            } else {
                const int gm = ws_blocks(k.cus, (f.Co + 63) / 64);
                long long r = 0;
                row = ws_flat_tile(f.N, f.H, f.W, gm, &r);
                if (f.mask) {      // (activation mask: the 16 x 16 tile form has the 2 KB of LDS left for the mask bytes)
                    row = WS_16x16;
                    r = ws_rounds(f.N, f.H, f.W, 16, 16, gm);
                }
                // 14 x 14 tiles in 224 rows where the image is made of them: the time of a launch is its rounds x the MFMA rows of
                // a tile, so the choice minimises that product (ties stay) at the measured levels.  A launch that takes statistics
                // keeps them bit for bit only with one tile per 14 x 14 image, so at 28^2 and 56^2 the forwards stay on 16 x 16 tiles:
                // another summation order moves the training step's outputs by per cents
                const bool same_stats = !f.stats || f.W == 14;
                const unsigned level = f.W == 14 ? 1u : f.W == 28 ? 2u : f.W == 56 ? 4u : 0u;
                if (can14 && same_stats && f.H == f.W && (k.levels14 & level) &&
                    ws_rounds(f.N, f.H, f.W, 14, 14, gm) * WS_TILES[WS_14x14].BM < r * WS_TILES[row].BM)
                    row = WS_14x14;
            }
        }
        if (row > WS_14x14) return c;
        // the tall form: images no wider than its tile, input and output of one size
        if (row == WS_TALL && (f.W > WS_TILES[WS_TALL].WT || f.Hi != f.H || f.Wi != f.W)) return c;
        c.form = f.mask ? WS_MASK : f.ep ? WS_EP : (!f.stats && !f.dbg && k.nostats) ? WS_NOSTATS : f.dbg ? WS_DBG : WS_STATS;
    }
    const WsTile& t = WS_TILES[row];
    // Which order of the store rows serves a launch ("fprop_dma_epi": -1 = the row's default, tools/wsepi_bench.py,
    // profiles/wsepi_ab.txt): WsEpi where the row has it, but for the affine epilogue
    c.epi = t.epi_forms != 0u && !f.ep && k.epi != 0;
    if (!(((c.epi ? t.epi_forms : t.forms) >> c.form) & 1u)) return c;      // (a mask on a tile without the LDS for its bytes, ...)
    c.ks = ws_ksplit(f, k, t);
    c.ks_form = f.stats || !k.nostats ? WS_KS_STATS : WS_KS_NOSTATS;
    c.row = row;
    return c;
}

// ---- conv_fprop_rw_kernel -------------------------------------------------------------------------------------------------------
// RwCfg<BN, NS, NSW, R, WT>: output channels of a block, ring stages by what the resident weights leave of the 160 KiB, store waves,
// pixel tile.  96-channel outputs (the data gradient of the 96 -> 32 concat layer: 53 KiB of staging beside 55 KiB of weights): a
// two-stage ring and no BatchNorm statistics (twelve chunks per row do not divide the store threads; a data gradient has none)
struct RwTile {
    int BN, NS, NSW, R, WT;
};
enum { RW_NROWS = 8, RW_NONE = -1 };
static constexpr RwTile RW_TILES[RW_NROWS] = {
    {32, 5, 4, 8, 32}, {32, 4, 4, 8, 32}, {32, 3, 4, 8, 32},        // Co <= 32 on wide images, NCH = 1, 2, 3
    {32, 5, 4, 16, 16}, {32, 4, 4, 16, 16}, {32, 3, 4, 16, 16},     // Co <= 32
    {64, 3, 4, 16, 16}, {96, 2, 2, 16, 16},
};
// The row for Co output channels behind NCH 32-channel chunks of input on images Wo wide.  8 x 32 pixel tiles on wide images: longer
// contiguous rows per fetch / store (224 x 224: 65 vs 69 us forward, 54 vs 58 data gradient); 16 x 16 wins at 112 x 112 (40 vs 45 us)
static inline int rw_select(int Co, int NCH, int Wo, bool stats) {
    if (NCH < 1 || NCH > 3 || Co > 96 || Wo < 12) return RW_NONE;
    if (Co <= 32) return (Wo >= 192 ? 0 : 3) + NCH - 1;
    if (Co <= 64) return 6;
    return stats ? RW_NONE : 7;
}
