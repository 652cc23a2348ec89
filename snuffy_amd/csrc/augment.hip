// Training augmentations on the device: what the reference does per crop on DataLoader workers with torchvision's PIL transforms
// (main_dino_adapter.py:674-745 DataAugmentationDINO; main_pretrain_adapter.py: RandomResizedCrop(224, (0.2, 1), bicubic) + flip +
// normalise) for a whole batch of decoded uint8 tiles, bit-identically to Pillow.
//
//   crop -> bicubic resize -> flip -> colour jitter (4 operations in a drawn order) -> grayscale -> Gaussian blur -> solarise
//        -> ToTensor + Normalize
// Every stage yields uint8 exactly as Pillow's does (augment_math.h holds the arithmetic); every decision is read from one 64-byte
// record per (view, image).  snf_augment_draw fills the records from Philox4x32-10; tests fill them by hand.
//
// Organisation.  One 256-thread workgroup owns one record from the crop to the fp32 store; a grid of at most two workgroups per CU
// walks the records.  A 224 x 224 x 3 view is 150 KB and its horizontally resized crop up to [H, S, 3], so neither is LDS-resident
// next to the other: the view lives as three uint8 planes in the workgroup's slot of a global workspace (L2-resident: a slot is
// written and re-read by one CU within microseconds), and LDS (48 KB, three workgroups per CU by LDS) holds what is re-read many
// times -- the strip of horizontally resized rows that a band of output rows needs, and the two tiles a three-pass box blur
// ping-pongs between.  The coefficient tables are built per record by the workgroup itself, in fp64, into its slot.
// No atomics; one owner per output element; integer sums only, so repeat calls are bit-identical.
#include "common.h"
#include "philox.h"
#include "augment_math.h"

namespace {

using namespace snf::aug;

constexpr int THREADS = 256;
constexpr int LDS_BYTES = 48 * 1024;   // >= 33 strip rows of 3 * 256 bytes; two blur tiles of 24 KB
constexpr int MAX_S = 256, MAX_HW = 1024, MAX_RATIO = 8;
constexpr float MAX_BLUR = 16.f;

__host__ __device__ inline size_t round16(size_t v) { return (v + 15) & ~(size_t)15; }
__host__ __device__ inline size_t table_bytes(int S, int kmax) { return round16(((size_t)4 * S + (size_t)2 * S * kmax) * sizeof(int)); }
__host__ __device__ inline size_t slot_bytes(int S, int kmax) { return table_bytes(S, kmax) + 3 * round16((size_t)S * S); }

int ksize_max(int h, int w, int S) {
    const double scale = (double)(h > w ? h : w) / (double)S;
    return (int)ceil(2.0 * (scale < 1.0 ? 1.0 : scale)) * 2 + 1;
}

int grid_for(int n) {
    int cus = snf::cu_count();
    if (cus < 1) cus = 256;
    return n < 2 * cus ? n : 2 * cus;
}

struct ApplyParams {
    const unsigned char* tiles;   // [b, h, w, 3]
    int b, h, w;
    const Record* recs;           // [n], record r crops tile r % b
    int n, S, kmax;
    unsigned char* ws;
    size_t slot;
    float* out;                   // [n, 3, S, S]
    float mean[3], std_[3];
};

__device__ __forceinline__ int block_sum(int v, int* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// jitter operations [k0, k1) of `order` and then (gray) the grayscale on every pixel of the planes, four pixels per thread and step;
// returns this thread's sum of L over the pixels it leaves behind (the contrast degenerate of the next operation)
__device__ __forceinline__ int pixel_pass(unsigned char* img, int PS, int npix, const Record& rec, int order, int k0, int k1, int mean,
                                          bool gray, bool store) {
    int sum = 0;
    for (int i4 = threadIdx.x; i4 < PS / 4; i4 += THREADS) {
        unsigned* p0 = reinterpret_cast<unsigned*>(img) + i4;
        unsigned* p1 = reinterpret_cast<unsigned*>(img + PS) + i4;
        unsigned* p2 = reinterpret_cast<unsigned*>(img + 2 * PS) + i4;
        const unsigned w0 = *p0, w1 = *p1, w2 = *p2;
        unsigned o0 = 0, o1 = 0, o2 = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            int r = (w0 >> (8 * e)) & 255, g = (w1 >> (8 * e)) & 255, b = (w2 >> (8 * e)) & 255;
            for (int k = k0; k < k1; ++k) {
                const int op = (order >> (2 * k)) & 3;
                jitter_op(op, op == 0 ? rec.f[0] : (op == 1 ? rec.f[1] : (op == 2 ? rec.f[2] : rec.f[3])), mean, &r, &g, &b);
            }
            const int l = luma(r, g, b);
            if (gray) r = g = b = l;
            if (4 * i4 + e < npix) sum += l;
            o0 |= (unsigned)r << (8 * e), o1 |= (unsigned)g << (8 * e), o2 |= (unsigned)b << (8 * e);
        }
        if (store) *p0 = o0, *p1 = o1, *p2 = o2;
    }
    return sum;
}

// Three extended box passes along the lines of one direction of one plane, a tile of lines at a time through LDS.
// vertical = false: lines are rows; true: lines are columns.  Within a tile the index that is contiguous in memory runs fastest.
__device__ __forceinline__ void blur_direction(unsigned char* plane, int S, Box box, bool vertical, unsigned char* lds) {
    const int nl = (LDS_BYTES / 2) / S < S ? (LDS_BYTES / 2) / S : S;
    unsigned char* buf[2] = {lds, lds + LDS_BYTES / 2};
    for (int l0 = 0; l0 < S; l0 += nl) {
        const int nlc = S - l0 < nl ? S - l0 : nl;
        const int sl = vertical ? 1 : S, sp = vertical ? nlc : 1, nfast = vertical ? nlc : S;
        for (int idx = threadIdx.x; idx < nlc * S; idx += THREADS) {
            const int slow = idx / nfast, fast = idx - slow * nfast;
            const int l = vertical ? fast : slow, p = vertical ? slow : fast;
            buf[0][l * sl + p * sp] = vertical ? plane[p * S + l0 + l] : plane[(l0 + l) * S + p];
        }
        __syncthreads();
#pragma unroll
        for (int pass = 0; pass < 3; ++pass) {
            const unsigned char* in = buf[pass & 1];
            unsigned char* out = buf[(pass + 1) & 1];
            for (int idx = threadIdx.x; idx < nlc * S; idx += THREADS) {
                const int slow = idx / nfast, fast = idx - slow * nfast;
                const int l = vertical ? fast : slow, p = vertical ? slow : fast;
                const unsigned char* line = in + l * sl;
                unsigned bulk = 0;
                for (int d = -box.r; d <= box.r; ++d) {
                    const int q = p + d;
                    bulk += line[(q < 0 ? 0 : (q >= S ? S - 1 : q)) * sp];
                }
                const int ql = p - box.r - 1, qr = p + box.r + 1;
                const unsigned edge = (unsigned)line[(ql < 0 ? 0 : ql) * sp] + (unsigned)line[(qr >= S ? S - 1 : qr) * sp];
                out[l * sl + p * sp] = (unsigned char)((bulk * box.ww + edge * box.fw + (1u << 23)) >> 24);
            }
            __syncthreads();
        }
        for (int idx = threadIdx.x; idx < nlc * S; idx += THREADS) {
            const int slow = idx / nfast, fast = idx - slow * nfast;
            const int l = vertical ? fast : slow, p = vertical ? slow : fast;
            (vertical ? plane[p * S + l0 + l] : plane[(l0 + l) * S + p]) = buf[1][l * sl + p * sp];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(THREADS) void augment_apply_kernel(ApplyParams P) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[LDS_BYTES];
    __shared__ int red[THREADS / 64];
    const int S = P.S, kmax = P.kmax, tid = threadIdx.x, npix = S * S, PS = (int)round16((size_t)npix);
    unsigned char* slot = P.ws + (size_t)blockIdx.x * P.slot;
    int* hb = reinterpret_cast<int*>(slot);   // [S][2] (first crop column, count), then the same for rows, then the coefficients
    int* vb = hb + 2 * S;
    int* hc = vb + 2 * S;                     // [S][kmax]
    int* vc = hc + S * kmax;
    unsigned char* img = slot + table_bytes(S, kmax);   // the view: 3 planes of PS bytes

    for (int r = blockIdx.x; r < P.n; r += gridDim.x) {
        Record rec = P.recs[r];
        // a table from the host was checked there, a drawn one is inside by construction: the clamps only keep a corrupt record in bounds
        rec.top = rec.top < 0 ? 0 : (rec.top > P.h - 1 ? P.h - 1 : rec.top);
        rec.left = rec.left < 0 ? 0 : (rec.left > P.w - 1 ? P.w - 1 : rec.left);
        rec.ch = rec.ch < 1 ? 1 : (rec.ch > P.h - rec.top ? P.h - rec.top : rec.ch);
        rec.cw = rec.cw < 1 ? 1 : (rec.cw > P.w - rec.left ? P.w - rec.left : rec.cw);
        int order = rec.order & 255;
        if (((1 << (order & 3)) | (1 << ((order >> 2) & 3)) | (1 << ((order >> 4) & 3)) | (1 << ((order >> 6) & 3))) != 15) order = 0xE4;
        const unsigned char* src = P.tiles + ((size_t)(r % P.b) * P.h + rec.top) * P.w * 3 + (size_t)rec.left * 3;

        // coefficient tables of this crop, one output pixel per thread
        for (int i = tid; i < 2 * S; i += THREADS) {
            if (i < S)
                coeff_row(rec.cw, S, i, kmax, hb + 2 * i, hc + i * kmax);
            else
                coeff_row(rec.ch, S, i - S, kmax, vb + 2 * (i - S), vc + (i - S) * kmax);
        }
        __syncthreads();

        // resize: bands of output rows; LDS holds the horizontally resized crop rows a band reads, [3][rows][S] uint8
        const int rows_cap = LDS_BYTES / (3 * S);
        for (int oy0 = 0; oy0 < S;) {
            const int y0 = vb[2 * oy0];
            int oy1 = oy0 + 1;
            while (oy1 < S && vb[2 * oy1] + vb[2 * oy1 + 1] - y0 <= rows_cap) ++oy1;
            int rows = vb[2 * (oy1 - 1)] + vb[2 * (oy1 - 1) + 1] - y0;
            rows = rows > rows_cap ? rows_cap : rows;
            for (int c = 0; c < 3; ++c)
                for (int idx = tid; idx < rows * S; idx += THREADS) {
                    const int y = idx / S, ox = idx - y * S;
                    const int xmin = hb[2 * ox], cnt = hb[2 * ox + 1];
                    const int* k = hc + ox * kmax;
                    const unsigned char* line = src + ((size_t)(y0 + y) * P.w + xmin) * 3 + c;
                    int ss = 1 << (PRECISION_BITS - 1);
                    for (int x = 0; x < cnt; ++x) ss += (int)line[3 * x] * k[x];
                    lds[c * rows * S + idx] = (unsigned char)clip8(ss >> PRECISION_BITS);
                }
            __syncthreads();
            const int band = oy1 - oy0;
            for (int c = 0; c < 3; ++c)
                for (int idx = tid; idx < band * S; idx += THREADS) {
                    const int oy = oy0 + idx / S, ox = idx - (oy - oy0) * S;
                    const int ymin = vb[2 * oy] - y0;
                    int cnt = vb[2 * oy + 1];
                    cnt = ymin + cnt > rows ? rows - ymin : cnt;
                    const int* k = vc + oy * kmax;
                    const unsigned char* col = lds + (c * rows + ymin) * S + ox;
                    int ss = 1 << (PRECISION_BITS - 1);
                    for (int y = 0; y < cnt; ++y) ss += (int)col[y * S] * k[y];
                    img[c * PS + oy * S + (rec.flip ? S - 1 - ox : ox)] = (unsigned char)clip8(ss >> PRECISION_BITS);
                }
            __syncthreads();
            oy0 = oy1;
        }

        // colour jitter and grayscale.  Contrast blends with the mean L of the image it meets, so the operations before it
        // run in one pass that also sums L, and contrast, the operations after it and the grayscale in a second pass.
        if (rec.jitter) {
            int cpos = 0;
            while (((order >> (2 * cpos)) & 3) != OP_CONTRAST) ++cpos;
            const int sum = block_sum(pixel_pass(img, PS, npix, rec, order, 0, cpos, 0, false, cpos > 0), red);
            const int mean = (2 * sum + npix) / (2 * npix);
            pixel_pass(img, PS, npix, rec, order, cpos, 4, mean, rec.gray != 0, true);
        } else if (rec.gray) {
            pixel_pass(img, PS, npix, rec, order, 0, 0, 0, true, true);
        }
        __syncthreads();

        if (rec.blur > 0.f) {
            Box box = gaussian_box(rec.blur < MAX_BLUR ? rec.blur : MAX_BLUR);
            box.r = box.r > S ? S : box.r;
            for (int dir = 0; dir < 2; ++dir)
                for (int c = 0; c < 3; ++c) blur_direction(img + c * PS, S, box, dir == 1, lds);
        }

        // solarise, ToTensor, Normalize: the expression of snf_tile_preprocess_u8
        for (int c = 0; c < 3; ++c) {
            float* dst = P.out + ((size_t)r * 3 + c) * npix;
            const float mean = P.mean[c], sd = P.std_[c];
            for (int i = tid; i < npix; i += THREADS) {
                int v = img[c * PS + i];
                if (rec.solar) v = v < 128 ? v : 255 - v;
                dst[i] = ((float)v / 255.0f - mean) / sd;
            }
        }
        __syncthreads();   // the slot is free for the next record
    }
}

struct DrawParams {
    const unsigned long long* state;   // {seed, offset}
    double pol[MAX_VIEWS * POLICY_WORDS];
    int views, b, h, w;
    Record* recs;                      // [views * b]
};

__global__ __launch_bounds__(THREADS) void augment_draw_kernel(DrawParams P) {
    const int r = blockIdx.x * THREADS + threadIdx.x;
    if (r >= P.views * P.b) return;
    const unsigned long long seed = P.state[0], off = P.state[1];
    auto rng = [&](int block, unsigned* o) {
        const snf::philox_u4 x = snf::philox4x32_10(snf::philox_u4{(unsigned)r, (unsigned)block, (unsigned)off, (unsigned)(off >> 32)},
                                                    (unsigned)seed, (unsigned)(seed >> 32));
        o[0] = x[0], o[1] = x[1], o[2] = x[2], o[3] = x[3];
    };
    Record rec;
    draw_record(rng, P.pol + (r / P.b) * POLICY_WORDS, P.h, P.w, &rec);
    P.recs[r] = rec;
}

}  // namespace

extern "C" {

size_t snf_augment_workspace_bytes(int h, int w, int size, int n_records) {
    if (h < 1 || w < 1 || size < 1 || size > MAX_S || n_records < 1) return 0;
    return (size_t)grid_for(n_records) * slot_bytes(size, ksize_max(h, w, size));
}

int snf_augment_draw(const void* state, const double* policies, int views, int b, int h, int w, void* records, snf_stream_t stream) {
    SNF_REQUIRE(state && policies && records && (reinterpret_cast<uintptr_t>(state) & 7) == 0 && (reinterpret_cast<uintptr_t>(records) & 3) == 0,
                "snf_augment_draw: null / unaligned pointer");
    SNF_REQUIRE(views >= 1 && views <= MAX_VIEWS && b >= 1 && (int64_t)views * b < (1ll << 31) / 64 && h >= 1 && w >= 1 && h <= MAX_HW &&
                    w <= MAX_HW,
                "snf_augment_draw: bad arguments views=%d (<= %d) b=%d h=%d w=%d (<= %d)", views, MAX_VIEWS, b, h, w, MAX_HW);
    DrawParams P;
    P.state = reinterpret_cast<const unsigned long long*>(state);
    for (int i = 0; i < MAX_VIEWS * POLICY_WORDS; ++i) P.pol[i] = i < views * POLICY_WORDS ? policies[i] : 0.0;
    for (int v = 0; v < views; ++v) {
        const double* p = P.pol + v * POLICY_WORDS;
        SNF_REQUIRE(p[0] > 0.0 && p[0] <= p[1] && p[14] <= p[15] && p[15] <= (double)MAX_BLUR,
                    "snf_augment_draw: view %d: scale (%g, %g) or blur radii (%g, %g) out of range", v, p[0], p[1], p[14], p[15]);
    }
    P.views = views, P.b = b, P.h = h, P.w = w;
    P.recs = reinterpret_cast<Record*>(records);
    hipLaunchKernelGGL(augment_draw_kernel, dim3((unsigned)((views * b + THREADS - 1) / THREADS)), dim3(THREADS), 0, snf::as_stream(stream), P);
    return snf::check_launch("augment_draw_kernel");
}

int snf_augment_apply_u8(const void* tiles_u8, int b, int h, int w, const void* records, int n_records, int size, const float* mean,
                         const float* std_, float* out_f32, void* workspace, size_t workspace_bytes, snf_stream_t stream) {
    SNF_REQUIRE(tiles_u8 && records && mean && std_ && out_f32 && workspace, "snf_augment_apply_u8: null pointer");
    SNF_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0 && (reinterpret_cast<uintptr_t>(records) & 3) == 0,
                "snf_augment_apply_u8: unaligned workspace / records");
    SNF_REQUIRE(b >= 1 && h >= 1 && w >= 1 && size >= 1 && n_records >= 1 && n_records % b == 0 &&
                    (int64_t)n_records * 3 * size * size < (1ll << 40),
                "snf_augment_apply_u8: bad shape b=%d h=%d w=%d size=%d records=%d (a multiple of b)", b, h, w, size, n_records);
    if (size > MAX_S || h > MAX_HW || w > MAX_HW || h > MAX_RATIO * size || w > MAX_RATIO * size) {
        snf::set_error("snf_augment_apply_u8: %d x %d tiles -> %d is outside the kernel (size <= %d, tile sides <= %d and <= %d * size)", h, w,
                       size, MAX_S, MAX_HW, MAX_RATIO);
        return SNF_EUNSUPPORTED;
    }
    ApplyParams P;
    P.tiles = reinterpret_cast<const unsigned char*>(tiles_u8);
    P.b = b, P.h = h, P.w = w;
    P.recs = reinterpret_cast<const Record*>(records);
    P.n = n_records, P.S = size, P.kmax = ksize_max(h, w, size);
    P.ws = reinterpret_cast<unsigned char*>(workspace);
    P.slot = slot_bytes(size, P.kmax);
    const int grid = grid_for(n_records);
    if (workspace_bytes < (size_t)grid * P.slot) {
        snf::set_error("snf_augment_apply_u8: workspace of %zu bytes, %zu needed", workspace_bytes, (size_t)grid * P.slot);
        return SNF_EWORKSPACE;
    }
    P.out = out_f32;
    for (int c = 0; c < 3; ++c) P.mean[c] = mean[c], P.std_[c] = std_[c];
    hipLaunchKernelGGL(augment_apply_kernel, dim3((unsigned)grid), dim3(THREADS), 0, snf::as_stream(stream), P);
    return snf::check_launch("augment_apply_kernel");
}

}  // extern "C"
