// Weight ingest of the segmentation path: the reference's layouts -> the per-lane MFMA panels of every kernel family, the bf16 / fp16 number
// formats of the split modes, and the uploads.  Host code only: no kernel is launched or named here.
#include <cmath>
#include <cstdint>
#include <cstring>

#include "unet_host.h"

namespace oai {

int conv_kc(int variant) { return variant == 1 ? 16 : 8; }

// Wk[tap][cin][cout] of the equivalent correlation (Conv3d as is; ConvTranspose3d k3 s1 p1 = conv with
// the kernel flipped and in/out swapped).
std::vector<float> canonical_k3(const oai_layer_params& p) {
    std::vector<float> w((size_t)27 * p.cin * p.cout);
    for (int t = 0; t < 27; ++t)
        for (int ci = 0; ci < p.cin; ++ci)
            for (int co = 0; co < p.cout; ++co) {
                float v;
                if (p.kind == 0) v = p.weight_host[((size_t)co * p.cin + ci) * 27 + t];
                else v = p.weight_host[((size_t)ci * p.cout + co) * 27 + (26 - t)];   // flip all three axes
                w[((size_t)t * p.cin + ci) * p.cout + co] = v;
            }
    return w;
}

// Chunk `ch` of a k3 layer's K loop: the chunks of source 0 (C0 channels) come first, then those of source 1 (the skip tensor of a concat layer:
// C1 channels, at offset C0 of the layer's input channels).  cl0 = the chunk's first channel inside its source.
struct ChunkSrc {
    bool first;
    int Csrc, cofs, cl0;
    ChunkSrc(int ch, int C0, int C1, int KC) {
        const int nch0 = (C0 + KC - 1) / KC;
        first = ch < nch0; Csrc = first ? C0 : C1; cofs = first ? 0 : C0; cl0 = (first ? ch : ch - nch0) * KC;
    }
};

// Panel order = consumption order of conv3_igemm_f32: [cb][chunk][tap][kg][nr][lane] x float4, where the
// float4 of lane (half h, column j) holds channels 4h..4h+3 of the k-group for cout cb*64+nr*32+j.
std::vector<float> pack_conv3_panel(const std::vector<float>& wk, int C0, int C1, int Cout, int KC) {
    const int Cin = C0 + C1, KG = KC / 8;
    const int ncb = (Cout + 63) / 64, nch0 = (C0 + KC - 1) / KC, nch1 = (C1 + KC - 1) / KC;
    std::vector<float> out(((size_t)ncb * (nch0 + nch1) * 27 * KG * 2 + 2) * 64 * 4, 0.0f);   // +1 step of prefetch slack
    size_t o = 0;
    for (int cb = 0; cb < ncb; ++cb)
        for (int ch = 0; ch < nch0 + nch1; ++ch) {
            const ChunkSrc cs(ch, C0, C1, KC);
            for (int t = 0; t < 27; ++t)
                for (int kg = 0; kg < KG; ++kg)
                    for (int nr = 0; nr < 2; ++nr)
                        for (int lane = 0; lane < 64; ++lane)
                            for (int s = 0; s < 4; ++s, ++o) {
                                const int cl = cs.cl0 + kg * 8 + 4 * (lane >> 5) + s;
                                const int co = cb * 64 + nr * 32 + (lane & 31);
                                if (cl < cs.Csrc && co < Cout) out[o] = wk[((size_t)t * Cin + cs.cofs + cl) * Cout + co];
                            }
        }
    return out;
}

// Frequency f of the Winograd F(2,3) weight transform along x: g0..g2 = the three x taps of one (dz, dy, cin, cout)
static inline double wino_u(int f, double g0, double g1, double g2) { return f == 0 ? g0 : f == 1 ? 0.5 * (g0 + g1 + g2) : f == 2 ? 0.5 * (g0 - g1 + g2) : g2; }

// ... of tap row t = dz * 3 + dy, input channel ci, output channel co of wk, the weights first multiplied by `scale` (an exact power of two): formed in double,
// rounded to fp32 once
static inline float wino_weight(const std::vector<float>& wk, int f, int t, int Cin, int ci, int Cout, int co, double scale = 1.0) {
    const size_t i = ((size_t)(t * 3) * Cin + ci) * Cout + co, dx = (size_t)Cin * Cout;
    return (float)wino_u(f, wk[i] * scale, wk[i + dx] * scale, wk[i + 2 * dx] * scale);
}

// conv3_wino_f32 (unet_wino_f32.h): the x-transformed weights (wino_weight) per (dz, dy, cin, cout); layout [cout block 64][frequency 4][chunk of 8 channels][tap (dz, dy) 9][cout half 2][lane 64][4]: lane (column = lane & 31, k half =
// lane >> 5) holds channels 4 (lane >> 5) .. + 3 of cout 32 nr + column -- the B operands of four v_mfma_f32_32x32x2_f32 k-steps, like pack_conv3_panel.
std::vector<float> pack_wino_f32_panel(const std::vector<float>& wk, int C0, int C1, int Cout) {
    constexpr int KC = 8;
    const int Cin = C0 + C1;
    const int ncb = (Cout + 63) / 64, nch0 = (C0 + KC - 1) / KC, nch1 = (C1 + KC - 1) / KC;
    std::vector<float> out(((size_t)ncb * 4 * (nch0 + nch1) * 9 * 2 + 6) * 64 * 4, 0.0f);     // + three taps of prefetch slack
    size_t o = 0;
    for (int cb = 0; cb < ncb; ++cb)
        for (int f = 0; f < 4; ++f)
            for (int ch = 0; ch < nch0 + nch1; ++ch) {
                const ChunkSrc cs(ch, C0, C1, KC);
                for (int q = 0; q < 9; ++q)
                    for (int nr = 0; nr < 2; ++nr)
                        for (int lane = 0; lane < 64; ++lane)
                            for (int s = 0; s < 4; ++s, ++o) {
                                const int cl = cs.cl0 + 4 * (lane >> 5) + s;
                                const int co = cb * 64 + nr * 32 + (lane & 31);
                                if (cl < cs.Csrc && co < Cout) out[o] = wino_weight(wk, f, q, Cin, cs.cofs + cl, Cout, co);
                            }
            }
    return out;
}

static inline uint16_t f32_to_bf16_rne(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
static inline float bf16_to_f32(uint16_t b) {
    uint32_t u = (uint32_t)b << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

static inline uint16_t f32_to_f16_rne(float f) {            // IEEE binary16, round to nearest even, subnormals kept
    uint32_t u;
    memcpy(&u, &f, 4);
    const uint32_t sign = (u >> 16) & 0x8000u;
    u &= 0x7fffffffu;
    if (u >= 0x7f800000u) return (uint16_t)(sign | (u > 0x7f800000u ? 0x7e00u : 0x7c00u));
    if (u >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);                    // rounds to >= 65520 -> inf
    if (u < 0x33000001u) return (uint16_t)sign;                                 // < 2^-25 -> 0
    int e = (int)(u >> 23) - 127;
    uint32_t m = (u & 0x7fffffu) | 0x800000u;
    int shift = e < -14 ? (-14 - e) + 13 : 13;                                  // subnormal: extra shift
    uint32_t half = m >> shift, rem = m & ((1u << shift) - 1), mid = 1u << (shift - 1);
    if (rem > mid || (rem == mid && (half & 1))) ++half;
    uint32_t out = e < -14 ? half : (((uint32_t)(e + 15) << 10) + (half - 0x400u));   // carry propagates into the exponent
    return (uint16_t)(sign | out);
}
static inline float f16_to_f32(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
    uint32_t e = (h >> 10) & 31u, m = h & 0x3ffu, u;
    if (e == 0) {
        if (m == 0) u = sign;
        else { int s = 0; while (!(m & 0x400u)) { m <<= 1; ++s; } u = sign | ((uint32_t)(113 - s) << 23) | ((m & 0x3ffu) << 13); }
    } else if (e == 31) u = sign | 0x7f800000u | (m << 13);
    else u = sign | ((e + 112) << 23) | (m << 13);
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// Term `term` (0 = high, 1 = low, ...) of the fp16 split of r: every term is the RNE fp16 of what the terms before it left over
static inline uint16_t f16_term(float r, int term) {
    uint16_t b = 0;
    for (int kk = 0; kk <= term; ++kk) { b = f32_to_f16_rne(r); r -= f16_to_f32(b); }
    return b;
}

// Split-bf16 panel of conv3_igemm_bf16s: [cb][chunk of 16][tap][term][nr][lane] x 8 bf16, where lane (half h, column j)
// holds channels 8h..8h+7 of the chunk for cout cb*64+nr*32+j.  Terms: w = t0 + t1 (+ t2), each the RNE bf16 of the rest.
// fp16: `wscale[co]` (an exact power of two) multiplies every weight of output channel co before the split.
// `src1_factor` (an exact power of two) multiplies the weights of the source-1 (skip) channels: the two sources of a concat layer are stored
// with different activation exponents and the panel carries their ratio.
std::vector<float> pack_conv3_panel_bf(const std::vector<float>& wk, int C0, int C1, int Cout, int NS,
                                       bool fp16, const std::vector<float>* wscale, float src1_factor) {
    const int Cin = C0 + C1, KC = 16;
    const int ncb = (Cout + 63) / 64, nch0 = (C0 + KC - 1) / KC, nch1 = (C1 + KC - 1) / KC;
    const size_t units = ((size_t)ncb * (nch0 + nch1) * 27 + 1) * NS * 2 * 64;      // 16-byte units, +1 tap of prefetch slack
    std::vector<float> out(units * 4, 0.0f);
    uint16_t* o16 = reinterpret_cast<uint16_t*>(out.data());
    size_t u = 0;
    for (int cb = 0; cb < ncb; ++cb)
        for (int ch = 0; ch < nch0 + nch1; ++ch) {
            const ChunkSrc cs(ch, C0, C1, KC);
            for (int t = 0; t < 27; ++t)
                for (int k = 0; k < NS; ++k)
                    for (int nr = 0; nr < 2; ++nr)
                        for (int lane = 0; lane < 64; ++lane, ++u)
                            for (int j = 0; j < 8; ++j) {
                                const int cl = cs.cl0 + 8 * (lane >> 5) + j;
                                const int co = cb * 64 + nr * 32 + (lane & 31);
                                if (cl < cs.Csrc && co < Cout) {
                                    float r = wk[((size_t)t * Cin + cs.cofs + cl) * Cout + co] * (wscale ? (*wscale)[co] : 1.0f) * (cs.first ? 1.0f : src1_factor);
                                    uint16_t b = 0;
                                    for (int kk = 0; kk <= k && !fp16; ++kk) { b = f32_to_bf16_rne(r); r -= bf16_to_f32(b); }
                                    o16[u * 8 + j] = fp16 ? f16_term(r, k) : b;
                                }
                            }
        }
    return out;
}

// Tap of step j (0..13), lane half tsel, of conv3_igemm_sres<..., M16>: 27 taps = 13 pairs + 1 (see the kernel's header comment).  t = (dz * 3 + dy) * 3 + dx.
static inline int m16_step_tap(int j, int tsel) {
    if (j < 9) return 3 * j + tsel;                          // (q = j, dx 0) | (q, dx 1)
    if (j < 12) return 3 * (3 * (j - 9) + tsel) + 2;         // (q, dx 2) | (q + 1, dx 2), q = 0, 3, 6
    if (j == 12) return 3 * (2 + 3 * tsel) + 2;              // (2, dx 2) | (5, dx 2)
    return 26;                                               // (8, dx 2) alone
}

// Panel of conv3_igemm_sres<..., M16> (v_mfma_f32_16x16x32_f16, K = a PAIR of taps x 16 channels): [cb][chunk of 16][step 14][X' | Y'][n2 4][lane] x 8 fp16.
// Lane (column c = lane & 15, group g = lane >> 4) of tile n2 holds cout cb * 64 + n2 * 16 + c, channels 8 (g & 1) .. + 7 of tap m16_step_tap(j, g >> 1):
// X' = the HIGH terms b0 of both taps, Y' = the LOW terms b1.  Step 13 (the 27th tap alone, A = [a0 | a1]): X' = [b0 | b0], Y' = [b1 | 0].  The values are
// pack_conv3_panel_bf's fp16 terms (same scales, same split).  + 1 step of prefetch slack (the kernel requests one step past its last).
static std::vector<float> pack_conv3_m16_panel(const std::vector<float>& wk, int C0, int C1, int Cout, const std::vector<float>& wscale, float src1_factor) {
    const int Cin = C0 + C1, KC = 16;
    const int ncb = (Cout + 63) / 64, nch0 = (C0 + KC - 1) / KC, nch1 = (C1 + KC - 1) / KC;
    const size_t units = ((size_t)ncb * (nch0 + nch1) * 14 + 1) * 2 * 4 * 64;          // 16-byte units
    std::vector<float> out(units * 4, 0.0f);
    uint16_t* o16 = reinterpret_cast<uint16_t*>(out.data());
    size_t u = 0;
    for (int cb = 0; cb < ncb; ++cb)
        for (int ch = 0; ch < nch0 + nch1; ++ch) {
            const ChunkSrc cs(ch, C0, C1, KC);
            for (int j = 0; j < 14; ++j)
                for (int kind = 0; kind < 2; ++kind)             // 0: X', 1: Y'
                    for (int n2 = 0; n2 < 4; ++n2)
                        for (int lane = 0; lane < 64; ++lane, ++u) {
                            const int g = lane >> 4, tsel = g >> 1;
                            if (j == 13 && kind == 1 && tsel == 1) continue;           // step 13: Y' = [b1 | 0]
                            const int t = m16_step_tap(j, tsel), term = kind;
                            const int co = cb * 64 + n2 * 16 + (lane & 15);
                            if (co >= Cout) continue;
                            for (int e = 0; e < 8; ++e) {
                                const int cl = cs.cl0 + 8 * (g & 1) + e;
                                if (cl < cs.Csrc) o16[u * 8 + e] = f16_term(wk[((size_t)t * Cin + cs.cofs + cl) * Cout + co] * wscale[co] * (cs.first ? 1.0f : src1_factor), term);
                            }
                        }
        }
    return out;
}

// Panel of conv3_wino_sres (unet_wino.h): [cb][frequency f][chunk of 16][tap (dz, dy)][term][nr][lane] x 8 fp16, lane (half h, column j) =
// channels 8h..8h+7 of the chunk for cout cb*64+nr*32+j, of the x-transformed weights
//   u0 = g0, u1 = (g0 + g1 + g2) / 2, u2 = (g0 - g1 + g2) / 2, u3 = g2     (g = the three x taps of (dz, dy, cin, cout)),
// formed in double from the scaled weights (wscale, src1_factor: see pack_conv3_panel_bf), rounded to fp32 once, then split.
static std::vector<float> pack_wino_panel(const std::vector<float>& wk, int C0, int C1, int Cout, const std::vector<float>& wscale, float src1_factor) {
    const int Cin = C0 + C1, KC = 16;
    const int ncb = Cout / 64, nch0 = (C0 + KC - 1) / KC, nch1 = (C1 + KC - 1) / KC;
    const size_t units = ((size_t)ncb * 4 * (nch0 + nch1) * 9 + 2) * 2 * 2 * 64;      // 16-byte units, +2 taps of prefetch slack (one is read)
    std::vector<float> out(units * 4, 0.0f);
    uint16_t* o16 = reinterpret_cast<uint16_t*>(out.data());
    size_t u = 0;
    for (int cb = 0; cb < ncb; ++cb)
        for (int f = 0; f < 4; ++f)
            for (int ch = 0; ch < nch0 + nch1; ++ch) {
                const ChunkSrc cs(ch, C0, C1, KC);
                for (int t = 0; t < 9; ++t)                          // t = dz * 3 + dy
                    for (int k = 0; k < 2; ++k)
                        for (int nr = 0; nr < 2; ++nr)
                            for (int lane = 0; lane < 64; ++lane, ++u)
                                for (int j = 0; j < 8; ++j) {
                                    const int cl = cs.cl0 + 8 * (lane >> 5) + j;
                                    const int co = cb * 64 + nr * 32 + (lane & 31);
                                    if (cl < cs.Csrc) o16[u * 8 + j] = f16_term(wino_weight(wk, f, t, Cin, cs.cofs + cl, Cout, co, (double)wscale[co] * (cs.first ? 1.0 : (double)src1_factor)), k);
                                }
            }
    return out;
}

// Panel of conv3_wino_sres<.., M16> (v_mfma_f32_16x16x32_f16, K = a PAIR of taps x 16 channels): [cb][frequency f][chunk of 16][step 5][X' | Y'][n2 4][lane]
// x 8 fp16.  Lane (column c = lane & 15, group g = lane >> 4) of tile n2 holds cout cb * 64 + n2 * 16 + c, channels 8 (g & 1) .. + 7 of tap
// 2 j + (g >> 1) (steps j < 4): X' = the HIGH terms b0 of both taps, Y' = the LOW terms b1.  Step 4 (the ninth tap alone, A = [a0 | a1]):
// X' = [b0(8) | b0(8)], Y' = [b1(8) | 0].  The values are pack_wino_panel's (same transformed weights, same scales, same split).
static std::vector<float> pack_wino16_panel(const std::vector<float>& wk, int C0, int C1, int Cout, const std::vector<float>& wscale, float src1_factor) {
    const int Cin = C0 + C1, KC = 16;
    const int ncb = Cout / 64, nch0 = (C0 + KC - 1) / KC, nch1 = (C1 + KC - 1) / KC;
    const size_t units = ((size_t)ncb * 4 * (nch0 + nch1) * 5 + 2) * 2 * 4 * 64;       // 16-byte units, + 2 steps of prefetch slack
    std::vector<float> out(units * 4, 0.0f);
    uint16_t* o16 = reinterpret_cast<uint16_t*>(out.data());
    size_t u = 0;
    for (int cb = 0; cb < ncb; ++cb)
        for (int f = 0; f < 4; ++f)
            for (int ch = 0; ch < nch0 + nch1; ++ch) {
                const ChunkSrc cs(ch, C0, C1, KC);
                for (int j = 0; j < 5; ++j)
                    for (int kind = 0; kind < 2; ++kind)             // 0: X', 1: Y'
                        for (int n2 = 0; n2 < 4; ++n2)
                            for (int lane = 0; lane < 64; ++lane, ++u) {
                                const int g = lane >> 4, tsel = g >> 1;
                                int t, term;
                                if (j < 4) { t = 2 * j + tsel; term = kind; }
                                else { t = 8; term = kind; if (kind == 1 && tsel == 1) continue; }     // step 4: X' = [b0 | b0], Y' = [b1 | 0]
                                const int co = cb * 64 + n2 * 16 + (lane & 15);
                                for (int e = 0; e < 8; ++e) {
                                    const int cl = cs.cl0 + 8 * (g & 1) + e;
                                    if (cl < cs.Csrc) o16[u * 8 + e] = f16_term(wino_weight(wk, f, t, Cin, cs.cofs + cl, Cout, co, (double)wscale[co] * (cs.first ? 1.0 : (double)src1_factor)), term);
                                }
                            }
            }
    return out;
}

// [N/64][Cin/8][2][lane] x float4 for upconv2_igemm_f32; column n = parity*Cout + co
std::vector<float> pack_up_panel(const oai_layer_params& p) {
    const int N = 8 * p.cout, nnb = (N + 63) / 64, nkg = (p.cin + 7) / 8;
    std::vector<float> out((size_t)nnb * nkg * 2 * 64 * 4, 0.0f);
    size_t o = 0;
    for (int nb = 0; nb < nnb; ++nb)
        for (int kg = 0; kg < nkg; ++kg)
            for (int nr = 0; nr < 2; ++nr)
                for (int lane = 0; lane < 64; ++lane)
                    for (int s = 0; s < 4; ++s, ++o) {
                        const int ci = kg * 8 + 4 * (lane >> 5) + s;
                        const int col = nb * 64 + nr * 32 + (lane & 31);
                        if (ci < p.cin && col < N) {
                            const int par = col / p.cout, co = col % p.cout;
                            out[o] = p.weight_host[((size_t)ci * p.cout + co) * 8 + par];   // [ci][co][a][b][c]
                        }
                    }
    return out;
}

// split-fp16 panel of upconv2_igemm<true>: [N/64][Cin/16][term 2][nr 2][lane] x 8 fp16; lane (half h, column j) holds
// channels 16*ks + 8h .. +7 for column nb*64 + nr*32 + j (column n = parity*Cout + co); weights of output channel co are
// first multiplied by wscale[co] (exact power of two)
static std::vector<float> pack_up_panel_f16(const float* w /*[ci][co][8]*/, int cin, int cout, const std::vector<float>& wscale) {
    const int N = 8 * cout, nnb = (N + 63) / 64, nks = (cin + 15) / 16;
    std::vector<float> out((size_t)nnb * nks * 4 * 64 * 4, 0.0f);
    uint16_t* o16 = reinterpret_cast<uint16_t*>(out.data());
    size_t u = 0;
    for (int nb = 0; nb < nnb; ++nb)
        for (int ks = 0; ks < nks; ++ks)
            for (int k = 0; k < 2; ++k)
                for (int nr = 0; nr < 2; ++nr)
                    for (int lane = 0; lane < 64; ++lane, ++u)
                        for (int j = 0; j < 8; ++j) {
                            const int ci = ks * 16 + 8 * (lane >> 5) + j;
                            const int col = nb * 64 + nr * 32 + (lane & 31);
                            if (ci < cin && col < N) {
                                const int par = col / cout, co = col % cout;
                                o16[u * 8 + j] = f16_term(w[((size_t)ci * cout + co) * 8 + par] * wscale[co], k);
                            }
                        }
    return out;
}

template <typename T>
int upload(oai_unet* h, const std::vector<float>& v, T** dst) {
    void* d = nullptr;
    OAI_CHECK_HIP(hipMalloc(&d, v.size() * sizeof(float)));
    h->allocs.push_back(d);
    OAI_CHECK_HIP(hipMemcpy(d, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
    *dst = reinterpret_cast<T*>(d);
    return OAI_OK;
}
template int upload<float>(oai_unet*, const std::vector<float>&, float**);
template int upload<float4>(oai_unet*, const std::vector<float>&, float4**);

// (re)fill a device array that already exists (same size) or create it
template <typename T>
static int upload_into(oai_unet* h, const std::vector<float>& v, T** dst) {
    if (!*dst) return upload(h, v, dst);
    OAI_CHECK_HIP(hipMemcpy(*dst, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
    return OAI_OK;
}

// The Winograd panel of layer k (k3 layers with whole blocks of 64 couts) for the weight scales / skip exponent of its current fp16 panel
int pack_wino_layer(oai_unet* h, int k) {
    Layer& L = h->L[k];
    if (L.kind == 2 || L.wk_host.empty() || L.cout % 64 != 0 || L.ws.empty()) return OAI_OK;
    const std::vector<float> panel = pack_wino_panel(L.wk_host, L.c0, L.c1, L.cout, L.ws, ldexpf(1.0f, L.rel1));
    if (L.panel_wino && panel.size() != L.panel_wino_floats) return set_error(OAI_ERR_ARG, "Winograd panel of layer %d changed size", k);
    L.panel_wino_floats = panel.size();
    if (int rc = upload_into(h, panel, &L.panel_wino)) return rc;
    const std::vector<float> p16 = pack_wino16_panel(L.wk_host, L.c0, L.c1, L.cout, L.ws, ldexpf(1.0f, L.rel1));
    if (L.panel_wino16 && p16.size() != L.panel_wino16_floats) return set_error(OAI_ERR_ARG, "16x16x32 Winograd panel of layer %d changed size", k);
    L.panel_wino16_floats = p16.size();
    return upload_into(h, p16, &L.panel_wino16);
}

// The fp16 panel of layer k (k3 conv or k2s2 up-conv) for the current activation exponents.  Every output channel's weights are scaled
// by the power of two that puts max|w| in [2^7, 2^8) -- exact, undone by the epilogue scale -- so that the low split term of all
// weights down to 2^-11 of the largest stays in fp16's normal range.
int pack_fp16_layer(oai_unet* h, int k) {
    Layer& L = h->L[k];
    const int s1 = layer_src1(k);
    const int rel1 = s1 >= 0 ? h->act_exp[layer_src0(k)] - h->act_exp[s1] : 0;
    const float f1 = ldexpf(1.0f, rel1);
    L.ws.assign(L.cout, 1.0f);
    std::vector<float> panel;
    if (L.kind == 2) {
        for (int co = 0; co < L.cout; ++co) {
            float amax = 0.0f;
            for (int ci = 0; ci < L.cin; ++ci)
                for (int q = 0; q < 8; ++q) amax = fmaxf(amax, fabsf(L.wk_host[((size_t)ci * L.cout + co) * 8 + q]));
            if (amax > 0.0f && std::isfinite(amax)) { int e; frexpf(amax, &e); L.ws[co] = ldexpf(1.0f, 8 - e); }   // amax = m 2^e, m in [0.5,1)
        }
        panel = pack_up_panel_f16(L.wk_host.data(), L.cin, L.cout, L.ws);
    } else {
        const int Cin = L.c0 + L.c1;
        const size_t per = L.wk_host.size() / L.cout;                 // index i = tap * Cin + ci
        for (int co = 0; co < L.cout; ++co) {
            float amax = 0.0f;
            for (size_t i = 0; i < per; ++i)
                amax = fmaxf(amax, fabsf(L.wk_host[i * L.cout + co]) * ((int)(i % Cin) >= L.c0 ? f1 : 1.0f));
            if (amax > 0.0f && std::isfinite(amax)) { int e; frexpf(amax, &e); L.ws[co] = ldexpf(1.0f, 8 - e); }
        }
        panel = pack_conv3_panel_bf(L.wk_host, L.c0, L.c1, L.cout, 2, true, &L.ws, f1);
    }
    if (L.panel_bf[2] && panel.size() != L.panel_f16_floats) return set_error(OAI_ERR_ARG, "fp16 panel of layer %d changed size", k);
    L.panel_f16_floats = panel.size();
    L.rel1 = rel1;
    if (int rc = upload_into(h, panel, &L.panel_bf[2])) return rc;
    if (L.kind != 2) {                                               // the same terms in the order of the 16x16x32 tap pairs (conv3_igemm_sres<..., M16>)
        const std::vector<float> p16 = pack_conv3_m16_panel(L.wk_host, L.c0, L.c1, L.cout, L.ws, f1);
        if (L.panel_m16 && p16.size() != L.panel_m16_floats) return set_error(OAI_ERR_ARG, "16x16x32 panel of layer %d changed size", k);
        L.panel_m16_floats = p16.size();
        if (int rc = upload_into(h, p16, &L.panel_m16)) return rc;
    }
    return (h->opt_wino || L.panel_wino) ? pack_wino_layer(h, k) : OAI_OK;
}

// The fp16x3 epilogue arrays of every layer for the current activation exponents (see Layer::scale_f16).  ec0 reads the raw volume
// (exponent 0) and has no panel; dc0 reads dc1's records and produces logits (exponent 0): its weights carry 2^-e(dc1).
int refresh_fp16_affine(oai_unet* h) {
    for (int k = 0; k < 17; ++k) {
        Layer& L = h->L[k];
        const int e_out = h->act_exp[k], e_in = k == EC0 ? 0 : h->act_exp[layer_src0(k)];
        std::vector<float> sc(L.cout), sh(L.cout);
        for (int co = 0; co < L.cout; ++co) {
            const float ws = L.ws.empty() ? 1.0f : L.ws[co];
            sc[co] = ldexpf(L.scale_host[co] / ws, e_out - e_in);
            sh[co] = ldexpf(L.shift_host[co], e_out);
        }
        if (int rc = upload_into(h, sc, &L.scale_f16)) return rc;
        if (int rc = upload_into(h, sh, &L.shift_f16)) return rc;
    }
    Layer& H = h->L[DC0];
    std::vector<float> w(H.plain_host.size());
    for (size_t i = 0; i < w.size(); ++i) w[i] = ldexpf(H.plain_host[i], -h->act_exp[DC1]);
    return upload_into(h, w, &H.plain_f16);
}

}  // namespace oai
