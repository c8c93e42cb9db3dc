// The strided row copy shared by var_rollout_move (rollout.hip: destinations the host computed), var_rollout_move_at
// (env_step.hip: destinations a device word selects) and var_rollout_move_cursor (ppo_step.hip: the index list a device word
// selects): the segment table that travels to the kernel by value, the host code that
// checks and plans one segment, and the device code that moves one 16-byte piece.
#pragma once
#include "var_common.h"

namespace var_move {

constexpr int kThreads = 256;

// A row is cut into 16-byte pieces, one per thread.  Rows of 256 pieces or more take ceil(pieces / 256) workgroups each; shorter
// rows share a workgroup (256 / pieces of them).  gran: what both ends, the length and every stride are multiples of -- 16: one
// 16-byte load and store per piece, 4: up to four words, 1: up to sixteen bytes.
struct MoveSeg {
    const char* src; char* dst;
    long row_bytes, st, dt, se, de;     // strides in bytes: time (src, dst), env (src, dst)
    long rows;                          // n_t * n_env
    int ppr, rpb, cpr, gran;            // pieces per row, rows per workgroup, workgroups per row (one of rpb / cpr is 1)
    unsigned blk0;                      // first workgroup of this segment
};
struct MoveTable { MoveSeg s[VAR_MOVE_MAX_SEGS]; int n; };

// The segment workgroup `b` belongs to.
__device__ __forceinline__ int move_segment_of(const MoveTable& tab, unsigned b) {
    int si = 0;
#pragma unroll
    for (int i = 1; i < VAR_MOVE_MAX_SEGS; ++i) si += (i < tab.n && b >= tab.s[i].blk0) ? 1 : 0;
    return si;
}

// This thread's piece of segment `sg` (workgroup `b` of the launch), its destination shifted by dst_off bytes.
__device__ __forceinline__ void move_piece(const MoveSeg& sg, unsigned b, const int* __restrict__ ind, int n_env, int n_src_env,
                                           long dst_off) {
    const long lb = (long)(b - sg.blk0);
    const int tid = threadIdx.x;
    long row, piece;
    if (sg.cpr > 1) { row = lb / sg.cpr; piece = (lb % sg.cpr) * kThreads + tid; }
    else            { const int rl = tid / sg.ppr; row = lb * sg.rpb + rl; piece = tid % sg.ppr; if (rl >= sg.rpb) return; }
    if (row >= sg.rows || piece >= sg.ppr) return;
    const long t = row / n_env, j = row % n_env;
    const long e = ind ? (long)ind[j] : j;
    if (e < 0 || e >= n_src_env) return;                        // an index outside the source: that row is left alone
    const long off = piece * 16, left = sg.row_bytes - off;     // left >= 1
    const char* s = sg.src + t * sg.st + e * sg.se + off;
    char* d = sg.dst + dst_off + t * sg.dt + j * sg.de + off;
    if (sg.gran == 16) {
        *(uint4*)d = *(const uint4*)s;
    } else if (sg.gran == 4) {
        const int nw = left >= 16 ? 4 : (int)(left >> 2);
        unsigned w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) if (k < nw) w[k] = ((const unsigned*)s)[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) if (k < nw) ((unsigned*)d)[k] = w[k];
    } else {
        const int nb = left >= 16 ? 16 : (int)left;
        unsigned char w[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) if (k < nb) w[k] = ((const unsigned char*)s)[k];
#pragma unroll
        for (int k = 0; k < 16; ++k) if (k < nb) ((unsigned char*)d)[k] = w[k];
    }
}

inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const char *p = (const char*)a, *q = (const char*)b;
    return p < q + nb && q < p + na;
}

// Checks segment i of entry `who` and plans it into g behind `blocks` workgroups; sext / dext: the bytes from its first to its
// last source / destination byte.  extra_bits: further byte counts the piece width has to divide (a slot stride).
// VAR_OK, or VAR_ERR_ARG with the context's message set.
inline int move_plan_seg(var_ctx* c, const char* who, int i, const var_move_seg& u, int n_env, int n_src_env,
                         unsigned long long extra_bits, MoveSeg& g, unsigned long long& blocks, size_t& sext, size_t& dext) {
    if (!u.src || !u.dst || u.row_bytes < 1 || u.n_t < 1 || u.src_t_stride < 0 || u.dst_t_stride < 0 || u.src_env_stride < 0 ||
        u.dst_env_stride < 0 || u.n_t > (1L << 31) || u.row_bytes > (1L << 40)) {
        VAR_SET_ERR(c, "%s: segment %d: NULL end, row_bytes / n_t < 1 or a negative stride", who, i);
        return VAR_ERR_ARG;
    }
    // destination rows in their natural order: an env's row ends before the next one's starts, a step's rows before the next step's
    if ((n_env > 1 && u.dst_env_stride < u.row_bytes) ||
        (u.n_t > 1 && u.dst_t_stride < (long)(n_env - 1) * u.dst_env_stride + u.row_bytes)) {
        VAR_SET_ERR(c, "%s: segment %d: destination rows overlap each other", who, i);
        return VAR_ERR_ARG;
    }
    sext = (size_t)((u.n_t - 1) * u.src_t_stride + (long)(n_src_env - 1) * u.src_env_stride + u.row_bytes);
    dext = (size_t)((u.n_t - 1) * u.dst_t_stride + (long)(n_env - 1) * u.dst_env_stride + u.row_bytes);
    g.src = (const char*)u.src; g.dst = (char*)u.dst;
    g.row_bytes = u.row_bytes; g.st = u.src_t_stride; g.dt = u.dst_t_stride; g.se = u.src_env_stride; g.de = u.dst_env_stride;
    g.rows = u.n_t * (long)n_env;
    const unsigned long long bits = (uintptr_t)u.src | (uintptr_t)u.dst | (unsigned long long)u.row_bytes | (unsigned long long)u.src_t_stride |
                                    (unsigned long long)u.dst_t_stride | (unsigned long long)u.src_env_stride |
                                    (unsigned long long)u.dst_env_stride | extra_bits;
    g.gran = (bits & 15) == 0 ? 16 : ((bits & 3) == 0 ? 4 : 1);
    const long ppr = (u.row_bytes + 15) / 16;
    g.ppr = (int)(ppr < (1L << 30) ? ppr : (1L << 30));
    if (ppr >= (1L << 30)) { VAR_SET_ERR(c, "%s: segment %d: row too long", who, i); return VAR_ERR_ARG; }
    if (ppr >= kThreads) { g.cpr = (int)((ppr + kThreads - 1) / kThreads); g.rpb = 1; }
    else                 { g.cpr = 1; g.rpb = kThreads / (int)ppr; }
    g.blk0 = (unsigned)blocks;
    blocks += g.cpr > 1 ? (unsigned long long)g.rows * g.cpr : (unsigned long long)((g.rows + g.rpb - 1) / g.rpb);
    if (blocks > 0x7fffffffull) { VAR_SET_ERR(c, "%s: more than 2^31 - 1 workgroups", who); return VAR_ERR_ARG; }
    return VAR_OK;
}

// The whole table of an indexed gather (var_rollout_move, var_rollout_move_cursor): every check of include/var_hip.h, the plan in
// `tab`, the launch's workgroups in `blocks`, each destination's extent in dext.  has_ind: an index list is given.
inline int move_plan_gather(var_ctx* c, const char* who, const var_move_seg* segs, int n_seg, bool has_ind, int n_env, int n_src_env,
                            MoveTable& tab, unsigned long long& blocks, size_t* dext) {
    if (!segs || n_seg < 1 || n_seg > VAR_MOVE_MAX_SEGS) {
        VAR_SET_ERR(c, "%s: %d segments (1..%d, table not NULL)", who, n_seg, VAR_MOVE_MAX_SEGS);
        return VAR_ERR_ARG;
    }
    if (n_env < 1 || n_src_env < 1 || (!has_ind && n_env > n_src_env)) {
        VAR_SET_ERR(c, "%s: n_env %d, n_src_env %d (>= 1; without an index list n_env <= n_src_env)", who, n_env, n_src_env);
        return VAR_ERR_ARG;
    }
    tab.n = n_seg;
    size_t sext[VAR_MOVE_MAX_SEGS];
    blocks = 0;
    for (int i = 0; i < n_seg; ++i) {
        const int rc = move_plan_seg(c, who, i, segs[i], n_env, n_src_env, 0, tab.s[i], blocks, sext[i], dext[i]);
        if (rc != VAR_OK) return rc;
    }
    for (int i = 0; i < n_seg; ++i) {
        for (int j = 0; j < n_seg; ++j) {
            if (overlap(segs[i].dst, dext[i], segs[j].src, sext[j]) || (i < j && overlap(segs[i].dst, dext[i], segs[j].dst, dext[j]))) {
                VAR_SET_ERR(c, "%s: the destination range of segment %d overlaps a range of segment %d", who, i, j);
                return VAR_ERR_ARG;
            }
        }
    }
    return VAR_OK;
}

}  // namespace var_move
