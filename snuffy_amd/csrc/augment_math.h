// The arithmetic of the training augmentations (augment.hip), one function per piece of Pillow it restates.  Everything here is
// plain integer / IEEE float code with no FMA contraction, so the same source gives the same bits on the host and on the device;
// snuffy_amd/augment.py and tests/augment_ref.py hold the numpy twins that the CPU tests pin against Pillow.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SNF_HD __host__ __device__ __forceinline__
#else
#define SNF_HD inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)   // blend, the HSV round trip and the coefficient tables round every multiply and add separately
#endif

namespace snf {
namespace aug {

// one (view, image) record: 16 words, RECORD_DTYPE of snuffy_amd/augment.py
struct Record {
    int top, left, ch, cw;          // crop box inside the tile
    int flip, jitter, order, gray;  // order: jitter operation k in bits 2k .. 2k + 1 (0 brightness 1 contrast 2 saturation 3 hue)
    float f[4];                     // factors, indexed by operation code
    float blur;                     // Gaussian radius, <= 0: no blur
    int solar, fallback, pad;       // fallback: the draw took the centred crop (information only)
};
static_assert(sizeof(Record) == 64, "record layout");

enum { OP_BRIGHTNESS = 0, OP_CONTRAST = 1, OP_SATURATION = 2, OP_HUE = 3 };
constexpr int PRECISION_BITS = 32 - 8 - 2;
constexpr int POLICY_WORDS = 20, MAX_VIEWS = 16, DRAW_TRIES = 10;
constexpr double LOG_RATIO_LO = -0.2876820724517809, LOG_RATIO_HI = 0.28768207245178085;   // log(3/4), log(4/3)

// ---- resize: Pillow's precompute_coeffs + normalize_coeffs_8bpc for the bicubic filter ------------------------------------------
SNF_HD double cubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// row xx of the table of in_size -> out_size: bounds[0..1] = (first input pixel, count <= kmax), coef[0 .. count)
SNF_HD void coeff_row(int in_size, int out_size, int xx, int kmax, int* bounds, int* coef) {
    const double scale = (double)in_size / (double)out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * filterscale, ss = 1.0 / filterscale;
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    int cnt = xmax - xmin;
    if (cnt > kmax) cnt = kmax;   // never taken for a box inside the tile: kmax is the ksize of the whole tile
    double ww = 0.0;
    for (int x = 0; x < cnt; ++x) ww += cubic((x + xmin - center + 0.5) * ss);
    for (int x = 0; x < cnt; ++x) {
        double w = cubic((x + xmin - center + 0.5) * ss);
        if (ww != 0.0) w /= ww;
        coef[x] = w < 0 ? (int)(-0.5 + w * (1 << PRECISION_BITS)) : (int)(0.5 + w * (1 << PRECISION_BITS));
    }
    bounds[0] = xmin, bounds[1] = cnt;
}

SNF_HD int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// ---- colour ---------------------------------------------------------------------------------------------------------------------
SNF_HD int luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// Image.blend(degenerate, image, f) on one band value
SNF_HD int blend(int deg, int img, float f) {
    const float t = (float)deg + f * (float)(img - deg);
    if (f >= 0.f && f <= 1.f) return (int)t;
    return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

SNF_HD void rgb_to_hsv(int r, int g, int b, int* uh, int* us, int* uv) {
    const int maxc = r > g ? (r > b ? r : b) : (g > b ? g : b), minc = r < g ? (r < b ? r : b) : (g < b ? g : b);
    *uv = maxc;
    if (minc == maxc) {
        *uh = *us = 0;
        return;
    }
    const float cr = (float)(maxc - minc), s = cr / (float)maxc;
    const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
    float h;
    if (r == maxc)
        h = bc - gc;
    else if (g == maxc)
        h = (float)(2.0 + (double)rc - (double)bc);
    else
        h = (float)(4.0 + (double)gc - (double)rc);
    const double t = (double)h / 6.0 + 1.0;   // in [5/6, 11/6]: fmod(t, 1) is t - floor(t), exactly
    h = (float)(t - floor(t));
    *uh = clip8((int)((double)h * 255.0));
    *us = clip8((int)((double)s * 255.0));
}

SNF_HD int round8(float x) { return clip8((int)floor((double)x + 0.5)); }   // halves away from zero (x >= 0 here)

SNF_HD void hsv_to_rgb(int uh, int us, int uv, int* r, int* g, int* b) {
    if (us == 0) {
        *r = *g = *b = uv;
        return;
    }
    const float h = (float)uh * 6.0f / 255.0f, fi = floorf(h), f = h - fi, fs = (float)us / 255.0f, v = (float)uv;
    const int p = round8(v * (1.0f - fs)), q = round8(v * (1.0f - fs * f)), t = round8(v * (1.0f - fs * (1.0f - f)));
    switch ((int)fi % 6) {
        case 0: *r = uv, *g = t, *b = p; break;
        case 1: *r = q, *g = uv, *b = p; break;
        case 2: *r = p, *g = uv, *b = t; break;
        case 3: *r = p, *g = q, *b = uv; break;
        case 4: *r = t, *g = p, *b = uv; break;
        default: *r = uv, *g = p, *b = q; break;
    }
}

SNF_HD int hue_shift(float f) { return (int)((double)f * 255.0) & 255; }   // (uint8)(int)(f * 255)

// one jitter operation on one pixel; mean: the contrast degenerate of the image the operation sees
SNF_HD void jitter_op(int op, float f, int mean, int* r, int* g, int* b) {
    if (op == OP_HUE) {
        int h, s, v;
        rgb_to_hsv(*r, *g, *b, &h, &s, &v);
        hsv_to_rgb((h + hue_shift(f)) & 255, s, v, r, g, b);
        return;
    }
    const int l = luma(*r, *g, *b);
    const int dr = op == OP_BRIGHTNESS ? 0 : (op == OP_CONTRAST ? mean : l);
    *r = blend(dr, *r, f), *g = blend(dr, *g, f), *b = blend(dr, *b, f);
}

// ---- blur: Pillow's GaussianBlur = 3 extended box passes per direction -----------------------------------------------------------
struct Box {
    int r;              // whole pixels on each side of the centre
    unsigned ww, fw;    // 24-bit weights of a window pixel and of the two pixels just outside
};

SNF_HD Box gaussian_box(float radius) {
    const float sigma2 = radius * radius / 3.f;
    const float big_l = (float)sqrt(12.0 * (double)sigma2 + 1.0);
    const float l = (float)floor(((double)big_l - 1.0) / 2.0);
    float a = (2.f * l + 1.f) * (l * (l + 1.f) - 3.f * sigma2);
    a /= 6.f * (sigma2 - (l + 1.f) * (l + 1.f));
    const float r = l + a;
    Box box;
    box.r = (int)r;
    box.ww = (unsigned)((float)(1 << 24) / (r * 2.f + 1.f));
    box.fw = ((1u << 24) - (unsigned)(2 * box.r + 1) * box.ww) / 2u;
    return box;
}

// ---- draws ------------------------------------------------------------------------------------------------------------------------
SNF_HD double unit(unsigned x) { return ((double)x + 0.5) * (1.0 / 4294967296.0); }                  // (0, 1), exact in fp64
SNF_HD bool bernoulli(unsigned x, double p) { return (double)x < p * 4294967296.0; }                  // p = 1: always
SNF_HD int below(unsigned x, int n) { return (int)(((unsigned long long)x * (unsigned long long)n) >> 32); }   // floor(x n / 2^32)
SNF_HD float between(unsigned x, double lo, double hi) { return (float)(lo + (hi - lo) * unit(x)); }

// Record r of a table from its policy row.  rng(block, out[4]) returns Philox block `block` of this record.
//   blocks 0 .. 9: crop try t = (area, log-aspect, top, left)     block 10: (flip, jitter applied, grayscale, blur applied)
//   block 11: (solarise, blur radius, permutation index, unused)   block 12: (brightness, contrast, saturation, hue) factors
template <class Rng>
SNF_HD void draw_record(Rng rng, const double* pol, int H, int W, Record* out) {
    unsigned x[4];
    Record rec;
    bool have = false;
    for (int t = 0; t < DRAW_TRIES && !have; ++t) {
        rng(t, x);
        const double area = (pol[0] + (pol[1] - pol[0]) * unit(x[0])) * ((double)H * (double)W);
        const double ratio = exp(LOG_RATIO_LO + (LOG_RATIO_HI - LOG_RATIO_LO) * unit(x[1]));
        const double cw = rint(sqrt(area * ratio)), ch = rint(sqrt(area / ratio));
        if (cw > 0.0 && cw <= (double)W && ch > 0.0 && ch <= (double)H) {
            rec.cw = (int)cw, rec.ch = (int)ch;
            rec.top = below(x[2], H - rec.ch + 1), rec.left = below(x[3], W - rec.cw + 1);
            have = true;
        }
    }
    rec.fallback = have ? 0 : 1;
    if (!have) {   // centred: the whole tile, or its largest part with aspect clamped to [3/4, 4/3]
        const double in_ratio = (double)W / (double)H;
        rec.cw = W, rec.ch = H;
        if (in_ratio < 0.75)
            rec.ch = (int)rint((double)W / 0.75);
        else if (in_ratio > 4.0 / 3.0)
            rec.cw = (int)rint((double)H * (4.0 / 3.0));
        rec.ch = rec.ch < 1 ? 1 : (rec.ch > H ? H : rec.ch);
        rec.cw = rec.cw < 1 ? 1 : (rec.cw > W ? W : rec.cw);
        rec.top = (H - rec.ch) / 2, rec.left = (W - rec.cw) / 2;
    }
    rng(DRAW_TRIES, x);
    rec.flip = bernoulli(x[0], pol[2]) ? 1 : 0;
    rec.jitter = bernoulli(x[1], pol[3]) ? 1 : 0;
    rec.gray = bernoulli(x[2], pol[12]) ? 1 : 0;
    const bool blur = bernoulli(x[3], pol[13]);
    rng(DRAW_TRIES + 1, x);
    rec.solar = bernoulli(x[0], pol[16]) ? 1 : 0;
    rec.blur = blur ? between(x[1], pol[14], pol[15]) : 0.f;
    const int k = below(x[2], 24);   // the k-th permutation of (0, 1, 2, 3) in lexicographic order
    unsigned left = 0x3210u, order = 0;   // the operations not yet placed, one per nibble, ascending
    for (int i = 0; i < 4; ++i) {
        const int d = i == 0 ? k / 6 : (i == 1 ? (k % 6) / 2 : (i == 2 ? k % 2 : 0));
        order |= ((left >> (4 * d)) & 3u) << (2 * i);
        left = (left & ((1u << (4 * d)) - 1u)) | ((left >> (4 * d + 4)) << (4 * d));
    }
    rec.order = (int)order;
    rng(DRAW_TRIES + 2, x);
    for (int i = 0; i < 4; ++i) rec.f[i] = between(x[i], pol[4 + 2 * i], pol[5 + 2 * i]);
    rec.pad = 0;
    *out = rec;
}

}  // namespace aug
}  // namespace snf
