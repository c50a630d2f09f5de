// floor_common.h — what the two floor-height kernels share (eval_floor_kernel in eval_metrics.h, amass_floor_kernel in
// amass_prep.h): the reference's thresholds, the joints with a contact channel, and the LDS layout of a sequence whose 2 T
// static-height samples stay in one workgroup's LDS.  No kernel is defined here, so both translation units may include it.
#pragma once
#include "common.h"

namespace evalm {

static constexpr int NJ = 22;
static constexpr int FRAME_BITS = 12;
static constexpr int MAX_T = 1 << FRAME_BITS;  // 4096 frames: 2 T samples of 4 + 4 + 4 bytes and the group tables fill 153 of 160 KiB
static constexpr int FC_THREADS = 1024;
static constexpr int FC_ELEMS = 2 * MAX_T / FC_THREADS;  // sorted samples per thread, at most
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

EG_D bool within_eps(float a, float b) { return fabs((double)a - (double)b) <= DB_EPS; }

}  // namespace evalm
