// The per-pair result block of the initialisation models (orbx_init.hip),
// which the reconstruction (orbx_reconstruct.hip) reads where a device-resident
// models run left it.
#pragma once

#include <cstdint>

#include "orbx_pack.h"

namespace orbx {

constexpr int kInitMaxIter = 1024;

struct InitHdr {
    int32_t n, best_h, best_f, pad0;
    float SH, SF, RH, pad1;
    float H21[9], F21[9], T1[9], T2[9];
    float norm[8];   // mean x, mean y, sX, sY of frame 1, then of frame 2
};

// One pair's inputs, as element offsets into the call's keypoint / match /
// count / draw arrays (device-resident form: the context's slot buffers).
struct InitPair {
    long long k1_off, k2_off, m_off, draw_off;
    int32_t n1, n2;       // used when cnt1 / cnt2 < 0
    int32_t cnt1, cnt2;   // index into the count array (slot), or -1
    int32_t max_iter;
    float sigma;
};

// Byte offsets inside one pair's result block.
struct InitLayout {
    long long stride;
    int o_pairs, o_xy, o_sets, o_Hn, o_Fn, o_H21, o_H12, o_F21, o_sh, o_sf, o_inh, o_inf;
    int M, cap;   // iterations and matches the block is sized for
};

inline InitLayout make_layout(int M, int cap)
{
    InitLayout L;
    BlockOffsets o;
    o.take(sizeof(InitHdr));
    L.o_pairs = o.take((long long)cap * 8);
    L.o_xy = o.take((long long)cap * 16);
    L.o_sets = o.take((long long)M * 32);
    L.o_Hn = o.take((long long)M * 36);
    L.o_Fn = o.take((long long)M * 36);
    L.o_H21 = o.take((long long)M * 36);
    L.o_H12 = o.take((long long)M * 36);
    L.o_F21 = o.take((long long)M * 36);
    L.o_sh = o.take((long long)M * 4);
    L.o_sf = o.take((long long)M * 4);
    L.o_inh = o.take(cap);
    L.o_inf = o.take(cap);
    L.stride = o.end;
    L.M = M;
    L.cap = cap;
    return L;
}

}  // namespace orbx
