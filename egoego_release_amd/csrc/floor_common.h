// floor_common.h — determine_floor_height_and_contacts (utils/data_utils/process_amass_dataset.py:160-338) for one sequence and
// one 1024-thread workgroup: the reference's thresholds, the joints with a contact channel, the LDS layout, and the seven steps
// themselves, floor_body<LONG>.  The two floor-height kernels (eval_floor_kernel in eval_metrics.h, amass_floor_kernel in
// amass_prep.h) clamp their sequence, describe it in a FloorSeq, pick the memory and call it.  Everything here is a device (or
// host) function, no kernel, so both translation units may include it.
//
// LONG = false: a sequence of at most MAX_T frames; its arrays live in LDS (floor_lds) and a sample's key is 32 bits,
// compacted index << 12 | frame.  LONG = true: up to MAX_LEN frames; the arrays live in global memory and the key is 64 bits,
// compacted index << 32 | frame.  Nothing else differs, so a sequence gives the same bits either way.
//
// Step by step (n = number of static toe samples, at most 2 L):
//   1. per frame, eight velocity flags (|p[t + 1] - p[t]| < 0.005 in fp64; the last frame repeats the one before it);
//   2. one block scan over the 2 L virtual entries (left toe frames, then right toe frames) compacts the static heights in the
//      reference's order; a sample carries (compacted index << SHIFT | frame);
//   3. bitonic sort by (height, compacted index) over the next power of two;
//   4. DBSCAN(eps = 0.005, min_samples = 3) on the sorted line.  A point is core when three points, itself included, lie within
//      eps: h[i + 2] - h[i] <= eps, or h[i] - h[i - 2] <= eps, or both neighbours within eps.  Two cores within eps of each other
//      have only cores between them (any point between them sees both), so a core opens a cluster exactly when its left
//      neighbour is not a core within eps: one more scan numbers the clusters left to right.  sklearn numbers them by first
//      appearance in input order, i.e. by the smallest compacted index among their cores: an atomic min per cluster and a
//      rank count give that order.  A non-core point within eps of a core is a border point; only its two sorted neighbours can
//      be such cores (a core two places away would make the point itself core), and it takes the lower-numbered cluster if both
//      are.  With min_samples = 3 that last case cannot arise (the point would see both cores and be core); the rule is kept
//      as stated.  Everything else is noise (-1).  Clusters are contiguous runs of the sorted line; the noise group is not.
//   5. group medians in fp32 ((a + b) * 0.5f of the two middle samples, numpy's mean of two): runs by position, noise by a scan;
//      floor = the smallest, the first group in label order (-1, 0, 1, ...) on a tie;
//   6. the discard test needs a group's median root height over its unique frames: a frame bit mask (atomic or), a scan to
//      gather the root heights, and a rank count for the middle ones.  It runs for the floor group and for the groups that pass
//      the two cheap tests (median height, size) only;
//   7. contacts from the velocity flags and the heights above floor_height (not the offset height).
#pragma once
#include "common.h"

namespace evalm {

static constexpr int NJ = 22;
static constexpr int FRAME_BITS = 12;
static constexpr int MAX_T = 1 << FRAME_BITS;  // 4096 frames: 2 T samples of 4 + 4 + 4 bytes and the group tables fill 153 of 160 KiB
static constexpr int MAX_LEN = 1 << 16;        // frames with the arrays in global memory: 2 * MAX_LEN samples, 128 per thread in a scan
static constexpr int FC_THREADS = 1024;
static constexpr int MT_THREADS = 256;
static constexpr int N_ACC = 11 + NJ;
static constexpr int N_METRICS = 13 + NJ;
static constexpr int HEAD = 15;

static constexpr double VEL_THRESH = 0.005;  // FLOOR_VEL_THRESH = CONTACT_VEL_THRESH
static constexpr double DB_EPS = 0.005;
static constexpr float TOE_H = 0.04f, ANKLE_H = 0.08f;  // CONTACT_TOE_HEIGHT_THRESH, CONTACT_ANKLE_HEIGHT_THRESH
static constexpr float TERRAIN_H = 0.04f, ROOT_H = 0.04f, FLOOR_OFFSET = 0.01f;
// the eight joints with a contact channel, toes first: bit k of a frame's flags belongs to contact_joint(k)
// (left / right toe base, foot, hand, leg of body_model/utils.py:5-8)
EG_HD constexpr int contact_joint(int k) { return k == 0 ? 10 : k == 1 ? 11 : k == 2 ? 7 : k == 3 ? 8 : k == 4 ? 20 : k == 5 ? 21 : k == 6 ? 4 : 5; }

// LDS layout for a given cap, shared by host and device
struct FloorLds {
    size_t sh, sp, lab, gmed, gsz, rootv, vf, mask, part, total;
};
EG_HD FloorLds floor_lds(int cap) {
    FloorLds l;
    size_t o = 0;
    l.sh = o;    o += (size_t)cap * 4;
    l.sp = o;    o += (size_t)cap * 4;
    l.lab = o;   o += (size_t)cap * 4;
    l.gmed = o;  o += ((size_t)cap / 2 + 2) * 4;
    l.gsz = o;   o += ((size_t)cap / 2 + 2) * 4;
    l.rootv = o; o += (size_t)cap / 2 * 4;
    l.mask = o;  o += ((size_t)cap / 64 + 1) * 4;
    l.part = o;  o += (size_t)FC_THREADS * 4;
    l.vf = o;    o += (size_t)cap / 2;
    l.total = (o + 15) / 16 * 16;
    return l;
}
// cap for sequences of at most `frames` frames in LDS: the power of two, at least 64, that holds their 2 * frames samples
inline int floor_cap(int frames) {
    int cap = 64;
    while (cap < 2 * frames) cap <<= 1;
    return cap;
}

EG_D bool within_eps(float a, float b) { return fabs((double)a - (double)b) <= DB_EPS; }

// A sample's sort key (compacted index << SHIFT | frame), and the 32-entry flag words a thread keeps across a scan
template <bool LONG>
struct Key {
    typedef uint32_t T;
    static constexpr int SHIFT = FRAME_BITS, SCAN_WORDS = 1;
};
template <>
struct Key<true> {
    typedef unsigned long long T;
    static constexpr int SHIFT = 32, SCAN_WORDS = 2 * MAX_LEN / FC_THREADS / 32;
};
static_assert(2 * MAX_T <= 32 * Key<false>::SCAN_WORDS * FC_THREADS && 2 * MAX_LEN <= 32 * Key<true>::SCAN_WORDS * FC_THREADS,
              "a scan over 2 L entries gives a thread at most 32 * SCAN_WORDS of them");

// the arrays of one sequence, in LDS or in global memory (part, the scan's partial sums, is in LDS always)
template <bool LONG>
struct FloorMem {
    float* sh;
    typename Key<LONG>::T* sp;
    int* lab;
    float* gmed;
    int* gsz;
    float* rootv;
    uint32_t* mask;
    uint8_t* vf;
    int* part;
};
EG_D FloorMem<false> floor_mem_lds(unsigned char* lds, int cap) {
    const FloorLds lay = floor_lds(cap);
    FloorMem<false> m;
    m.sh = (float*)(lds + lay.sh);
    m.sp = (uint32_t*)(lds + lay.sp);
    m.lab = (int*)(lds + lay.lab);
    m.gmed = (float*)(lds + lay.gmed);
    m.gsz = (int*)(lds + lay.gsz);
    m.rootv = (float*)(lds + lay.rootv);
    m.mask = (uint32_t*)(lds + lay.mask);
    m.vf = lds + lay.vf;
    m.part = (int*)(lds + lay.part);
    return m;
}

// one sequence as floor_body sees it: each kernel fills it from its own arguments
struct FloorSeq {
    const float* P;       // [L][22][3]: the sequence's first joint row
    int L, size_thresh;
    float* contacts;      // [contact_rows][22]; rows from L on are written as zeros
    int contact_rows;
    int* labels;          // [label_slots] in compacted order, -2 past n_static; or nullptr
    int label_slots;
    float *floor_h, *offset_h;            // the sequence's own result slots
    int *discard, *n_static, *n_groups;
};

// Exclusive prefix sum of flag(i), i < n, over the block: emit(i, prefix, flag(i)) for every i, returns the total.  A thread owns
// a contiguous run of ceil(n / threads) <= 32 * WORDS entries and evaluates each flag once, before any emit runs.
template <int WORDS, typename F, typename E>
EG_D int block_scan(int n, int* part, F flag, E emit) {
    const int tid = threadIdx.x, chunk = (n + FC_THREADS - 1) / FC_THREADS;
    const int lo = min(tid * chunk, n), hi = min(lo + chunk, n);
    uint32_t bits[WORDS];
    int cnt = 0;
#pragma unroll
    for (int w = 0; w < WORDS; ++w) {
        bits[w] = 0;
        const int s = lo + 32 * w, e = WORDS == 1 ? hi : min(s + 32, hi);
        for (int i = s; i < e; ++i) bits[w] |= (flag(i) ? 1u : 0u) << (i - s);
        cnt += __popc(bits[w]);
    }
    part[tid] = cnt;
    __syncthreads();
    for (int d = 1; d < FC_THREADS; d <<= 1) {
        const int v = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int pre = part[tid] - cnt;
    const int total = part[FC_THREADS - 1];
#pragma unroll
    for (int w = 0; w < WORDS; ++w) {
        const int s = lo + 32 * w, e = WORDS == 1 ? hi : min(s + 32, hi);
        for (int i = s; i < e; ++i) {
            const bool f = (bits[w] >> (i - s)) & 1u;
            emit(i, pre, f);
            pre += f;
        }
    }
    __syncthreads();
    return total;
}

// the median (fp32, numpy's) of the root heights of the unique frames of the samples labelled `label`
template <bool LONG>
EG_D float root_median(int label, int n, int L, const float* P, const FloorMem<LONG>& m, float* s_pair) {
    typedef typename Key<LONG>::T K;
    const int tid = threadIdx.x;
    for (int w = tid; w < (L + 31) / 32; w += FC_THREADS) m.mask[w] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += FC_THREADS)
        if (m.lab[i] == label) {
            const uint32_t f = (uint32_t)(m.sp[i] & (((K)1 << Key<LONG>::SHIFT) - 1));
            atomicOr(&m.mask[f >> 5], 1u << (f & 31));
        }
    __syncthreads();
    const int cnt = block_scan<Key<LONG>::SCAN_WORDS>(L, m.part, [&](int t) { return (m.mask[t >> 5] >> (t & 31)) & 1u; },
                                                      [&](int t, int pre, bool f) { if (f) m.rootv[pre] = P[(size_t)t * NJ * 3 + 2]; });
    for (int i = tid; i < cnt; i += FC_THREADS) {
        const float v = m.rootv[i];
        int r = 0;
        for (int j = 0; j < cnt; ++j) {
            const float u = m.rootv[j];
            r += (u < v || (u == v && j < i)) ? 1 : 0;
        }
        if (r == (cnt - 1) / 2) s_pair[0] = v;
        if (r == cnt / 2) s_pair[1] = v;
    }
    __syncthreads();
    const float med = (s_pair[0] + s_pair[1]) * 0.5f;
    __syncthreads();
    return med;
}

// Steps 1-7 for the sequence q on the arrays m; s_pair (two floats) and s_best are the calling kernel's, in LDS.
template <bool LONG>
EG_D void floor_body(const FloorSeq& q, const FloorMem<LONG>& m, float* s_pair, unsigned long long* s_best) {
    typedef typename Key<LONG>::T K;
    constexpr int SHIFT = Key<LONG>::SHIFT, WORDS = Key<LONG>::SCAN_WORDS;
    const int tid = threadIdx.x, L = q.L;
    const float* P = q.P;
    float* const sh = m.sh;
    K* const sp = m.sp;
    int* const lab = m.lab;
    float* const gmed = m.gmed;
    int* const gsz = m.gsz;
    uint8_t* const vf = m.vf;
    int* const part = m.part;

    // 1. velocity flags
    for (int t = tid; t < L; t += FC_THREADS) {
        uint32_t flags = 0;
        if (L >= 2) {
            const int tv = t + 1 < L ? t : L - 2;
            const float* p0 = P + (size_t)tv * NJ * 3;
            const float* p1 = p0 + NJ * 3;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int j = contact_joint(k);
                const double dx = (double)p1[3 * j] - (double)p0[3 * j], dy = (double)p1[3 * j + 1] - (double)p0[3 * j + 1],
                             dz = (double)p1[3 * j + 2] - (double)p0[3 * j + 2];
                if (sqrt(dx * dx + dy * dy + dz * dz) < VEL_THRESH) flags |= 1u << k;
            }
        }
        vf[t] = (uint8_t)flags;
    }
    __syncthreads();

    // 2. static toe heights, left frames then right frames
    const int n = block_scan<WORDS>(2 * L, part, [&](int e) { return e < L ? (vf[e] & 1u) : ((vf[e - L] >> 1) & 1u); },
                                    [&](int e, int pre, bool f) {
                                        if (!f) return;
                                        const int fr = e < L ? e : e - L;
                                        sh[pre] = P[(size_t)fr * NJ * 3 + 3 * (e < L ? 10 : 11) + 2];
                                        sp[pre] = ((K)(uint32_t)pre << SHIFT) | (K)(uint32_t)fr;
                                    });

    // 3. sort by (height, compacted index)
    int np2 = 2;
    while (np2 < n) np2 <<= 1;
    for (int i = n + tid; i < np2; i += FC_THREADS) {
        sh[i] = __builtin_inff();
        sp[i] = ~(K)0;
    }
    __syncthreads();
    for (int k = 2; k <= np2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < np2; i += FC_THREADS) {
                const int l = i ^ j;
                if (l > i) {
                    const float hi_ = sh[i], hl = sh[l];
                    const K pi = sp[i], pl = sp[l];
                    const bool gt = hi_ > hl || (hi_ == hl && pi > pl);
                    if (gt == ((i & k) == 0)) {
                        sh[i] = hl; sh[l] = hi_;
                        sp[i] = pl; sp[l] = pi;
                    }
                }
            }
            __syncthreads();
        }

    // 4. DBSCAN on the sorted line
    auto is_core = [&](int i) {
        const bool l1 = i >= 1 && within_eps(sh[i], sh[i - 1]), r1 = i + 1 < n && within_eps(sh[i], sh[i + 1]);
        return (l1 && r1) || (i >= 2 && within_eps(sh[i], sh[i - 2])) || (i + 2 < n && within_eps(sh[i], sh[i + 2]));
    };
    for (int i = tid; i < n; i += FC_THREADS) lab[i] = is_core(i) ? 1 : 0;
    __syncthreads();
    // raw cluster ids, left to right: lab[i] = id for a core, -1 otherwise
    const int Kc = block_scan<WORDS>(n, part, [&](int i) { return lab[i] && !(i >= 1 && lab[i - 1] && within_eps(sh[i], sh[i - 1])); },
                                     [&](int i, int pre, bool f) {
                                         // (lab[i] is read by the owner of i and of i + 1 only, both before any emit: block_scan)
                                         lab[i] = lab[i] ? pre + (f ? 1 : 0) - 1 : -1;
                                     });
    for (int k = tid; k < Kc; k += FC_THREADS) gsz[k] = 0x7fffffff;
    __syncthreads();
    for (int i = tid; i < n; i += FC_THREADS)
        if (lab[i] >= 0) atomicMin(&gsz[lab[i]], (int)(uint32_t)(sp[i] >> SHIFT));
    __syncthreads();
    {  // a cluster's number = how many clusters appear before it in input order; the ranks wait in gmed (free until step 5)
        int* rank = (int*)gmed;
        for (int k = tid; k < Kc; k += FC_THREADS) {
            const int mine = gsz[k];
            int r = 0;
            for (int o = 0; o < Kc; ++o) r += gsz[o] < mine ? 1 : 0;
            rank[k] = r;
        }
        __syncthreads();
        for (int k = tid; k < Kc; k += FC_THREADS) gsz[k] = rank[k];
        __syncthreads();
    }
    // A border point takes the lower-numbered of the (at most two) neighbouring cores within eps.  First the non-core points
    // only, stored as -(label + 2) so that an entry's sign, all a neighbour looks at, does not change; then every entry decodes.
    for (int i = tid; i < n; i += FC_THREADS) {
        if (lab[i] >= 0) continue;
        const int cl = i >= 1 && lab[i - 1] >= 0 && within_eps(sh[i], sh[i - 1]) ? gsz[lab[i - 1]] : -1;
        const int cr = i + 1 < n && lab[i + 1] >= 0 && within_eps(sh[i], sh[i + 1]) ? gsz[lab[i + 1]] : -1;
        const int fin = cl < 0 ? cr : (cr < 0 ? cl : min(cl, cr));
        if (fin >= 0) lab[i] = -(fin + 2);
    }
    __syncthreads();
    for (int i = tid; i < n; i += FC_THREADS) {
        const int v = lab[i];
        const int fin = v >= 0 ? gsz[v] : -v - 2;  // (-1 stays -1)
        lab[i] = fin;
        if (q.labels) q.labels[(uint32_t)(sp[i] >> SHIFT)] = fin;
    }
    if (q.labels)
        for (int i = n + tid; i < q.label_slots; i += FC_THREADS) q.labels[i] = -2;
    __syncthreads();

    // 5. group medians; slot g = label + 1 (slot 0: noise)
    for (int i = tid; i < n; i += FC_THREADS) {
        const int l = lab[i];
        if (l < 0) continue;
        if (i == 0 || lab[i - 1] != l) gsz[l + 1] = i;
        if (i == n - 1 || lab[i + 1] != l) ((int*)gmed)[l + 1] = i;
    }
    __syncthreads();
    for (int g = 1 + tid; g <= Kc; g += FC_THREADS) {
        const int s = gsz[g], c = ((int*)gmed)[g] - s + 1;
        gmed[g] = (sh[s + (c - 1) / 2] + sh[s + c / 2]) * 0.5f;
        gsz[g] = c;
    }
    const int nn = block_scan<WORDS>(n, part, [&](int i) { return lab[i] < 0; }, [&](int, int, bool) {});
    block_scan<WORDS>(n, part, [&](int i) { return lab[i] < 0; },
                      [&](int i, int pre, bool f) {
                          if (!f) return;
                          if (pre == (nn - 1) / 2) s_pair[0] = sh[i];
                          if (pre == nn / 2) s_pair[1] = sh[i];
                      });
    if (tid == 0) {
        gsz[0] = nn;
        gmed[0] = nn ? (s_pair[0] + s_pair[1]) * 0.5f : __builtin_inff();
        *s_best = ~0ull;
    }
    __syncthreads();

    float floor_h = 0.f;
    int discard = 0;
    if (n > 0) {
        for (int g = tid; g <= Kc; g += FC_THREADS)
            if (gsz[g] > 0) {
                uint32_t u = __float_as_uint(gmed[g]);
                u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // order-preserving
                atomicMin(s_best, ((unsigned long long)u << 32) | (uint32_t)g);
            }
        __syncthreads();
        const int gbest = (int)(*s_best & 0xffffffffu);
        floor_h = gmed[gbest];
        // 6. DISCARD_TERRAIN_SEQUENCES (:267-277)
        const float min_root = root_median<LONG>(gbest - 1, n, L, P, m, s_pair);
        for (int g = 0; g <= Kc && !discard; ++g) {
            if (gsz[g] == 0 || !(gmed[g] > floor_h + TERRAIN_H) || !(gsz[g] > q.size_thresh)) continue;
            const float rm = root_median<LONG>(g - 1, n, L, P, m, s_pair);
            if (rm > min_root + ROOT_H) discard = 1;
        }
    }
    if (tid == 0) {
        *q.floor_h = floor_h;
        *q.offset_h = n > 0 ? floor_h - FLOOR_OFFSET : 0.f;
        *q.discard = discard;
        *q.n_static = n;
        *q.n_groups = Kc + (nn > 0 ? 1 : 0);
    }

    // 7. contacts
    for (int t = tid; t < q.contact_rows; t += FC_THREADS) {
        uint32_t on = 0;
        if (t < L) {
            const uint32_t flags = vf[t];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int j = contact_joint(k);
                const float hgt = P[(size_t)t * NJ * 3 + 3 * j + 2] - floor_h;
                if (((flags >> k) & 1u) && hgt < (k < 2 ? TOE_H : ANKLE_H)) on |= 1u << j;
            }
        }
        for (int j = 0; j < NJ; ++j) q.contacts[(size_t)t * NJ + j] = (float)((on >> j) & 1u);
    }
}

}  // namespace evalm
