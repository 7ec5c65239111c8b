// The live range store (vbm_live_store_*): a range store with a fixed region per stream that takes appended runs of
// packets and drops the oldest when a region is full.  The rules are written once here, for the kernels of
// live_store.hip and for the host twin (vbm_host_live_store_*, capi_decoder.cpp).
//
// Layout.  Stream i owns packet slots [i * (MP + 1), i * (MP + 1) + MP] of the flat index arrays and bytes
// [i * stride, i * stride + MB) of the flat data; stride is MB rounded up to 16.  Its `count` retained packets lie at the
// front of both: packet t is slot i * (MP + 1) + t, bytes [offsets[slot], offsets[slot + 1]), absolute in the flat data,
// offsets[i * (MP + 1)] == i * stride always.  The spare slot MP holds the end of a full region's last packet, so the
// range and cut kernels read offsets[j], offsets[j + 1] of any packet as they do in a plain store.  Positions
// (out_start) are absolute: samples since the slot's last restart.
//
// An append of one entry (np packets, nb bytes of the caller's CSR) to a slot of n packets and B bytes:
//   vbml_plan_entry   refuses it (offsets that are no CSR inside the data: VBM_EINVAL; np > MP or nb > MB:
//                     VBM_LIVE_EBIG; the slot is untouched) or decides the trim, vbml_drop
//   compaction        of a trimmed slot: the retained entries and bytes move to the front (k_live_compact; memmove)
//   vbml_walk_entry   continues the index from the carried state over the new packets, packet after packet as
//                     k_run_plan does (gap marks, vbmd_blockin<HS>), writes their entries behind the retained ones,
//                     the new state, and the records the host reads back
//   payload copy      the entry's bytes, one contiguous run of the CSR, behind the retained bytes
// The carried state is what k_run_plan carries (W of the last valid packet, vbmd_blockin's sc and gp) and the sample
// count.  A gap mark sets sc = gp = -1 at once: a failed packet changes neither, so the mark reaches the next valid
// packet, in this append or a later one.
#pragma once
#include <string.h>

#include "decode.h"
#include "vorbis_mi355x.h"

struct vbml_slot {
    int lastW;                       // W of the last valid packet, -1: none since the restart
    int count;                       // retained packets
    int hasv;                        // one of them is valid
    int cls;                         // the slot's class in a store of a mixed decoder
    long long sc, gp;                // vbmd_blockin's sample count and granule position, -1: none yet
    long long at;                    // output samples since the restart: totals
    long long lo;                    // first_sample: out_end of the first retained valid packet; none: at
};

struct vbml_arrays {                 // a store's regions, in device memory or (the twin) in host memory
    int MP;                          // max_packets
    long long MB, stride;            // max_bytes; the bytes between two regions
    vbml_slot *slots;                // [S]
    uint8_t *data;                   // [S * stride]
    long long *offsets, *out_start;  // [S * (MP + 1)]
    int *status, *begin, *end;       // [S * (MP + 1)]
};

struct vbml_plan {                   // what an append does to one slot
    int sid, k0, k1;                 // the slot; the entry's packets [k0, k1) of the caller's CSR
    int status;                      // 0, VBM_EINVAL or VBM_LIVE_EBIG
    int drop, keep;                  // packets dropped from the front, packets retained
    int by;                          // bit 0: the packet cap made the trim, bit 1: the byte cap
    long long cut, kept;             // bytes dropped, bytes retained
};

struct vbml_back {                   // per entry, read back by the host
    int status, dropped, retained, by;
    long long first_sample, total, bytes;
};

VBMD_HD vbml_slot vbml_fresh(int cls)
{
    const vbml_slot s = {-1, 0, 0, cls, -1, -1, 0, 0};
    return s;
}

// The trim rule.  A slot holds n packets whose bytes end at off[0 .. n] (off does not decrease); np packets of nb bytes
// arrive, np <= MP and nb <= MB.  They fit: nothing is dropped.  Otherwise the fewest packets go from the front such that
// what remains is at most half of each capacity, and at most what the run leaves free (a run above half a capacity
// leaves less than half).
VBMD_HD int vbml_drop(int n, const long long *off, int np, long long nb, int MP, long long MB)
{
    if (n + np <= MP && off[n] - off[0] + nb <= MB) return 0;
    const int keep_p = MP / 2 < MP - np ? MP / 2 : MP - np;
    const long long keep_b = MB / 2 < MB - nb ? MB / 2 : MB - nb;
    int lo = n > keep_p ? n - keep_p : 0, hi = n;          // the fewest d in [lo, n] with off[n] - off[d] <= keep_b
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (off[n] - off[mid] <= keep_b) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// src_off [.. k1]: the caller's offsets, src_bytes the size of its data
VBMD_HD void vbml_plan_entry(const vbml_arrays &A, int sid, int k0, int k1, const long long *src_off,
                             long long src_bytes, vbml_plan &p)
{
    const long long *off = A.offsets + (long long)sid * (A.MP + 1);
    const int n = A.slots[sid].count;
    p.sid = sid;
    p.k0 = k0;
    p.k1 = k1;
    p.status = 0;
    p.drop = 0;
    p.keep = n;
    p.by = 0;
    p.cut = 0;
    p.kept = off[n] - off[0];
    bool csr = src_off[k0] >= 0 && src_off[k1] <= src_bytes;
    for (int k = k0; k < k1 && csr; k++) csr = src_off[k + 1] >= src_off[k];
    if (!csr) {
        p.status = VBM_EINVAL;
        return;
    }
    const int np = k1 - k0;
    const long long nb = src_off[k1] - src_off[k0];
    if (np > A.MP || nb > A.MB) {
        p.status = VBM_LIVE_EBIG;
        return;
    }
    p.drop = vbml_drop(n, off, np, nb, A.MP, A.MB);
    if (p.drop) p.by = (n + np > A.MP ? 1 : 0) | (p.kept + nb > A.MB ? 2 : 0);      // p.kept: still all n packets' bytes
    p.keep = n - p.drop;
    p.cut = off[p.drop] - off[0];
    p.kept = off[n] - off[p.drop];
}

// Behind the compaction.  head_status / head_W: vbmd_head's verdict on every packet of the caller's CSR (k_index_head).
// pk_status / pk_out_end [k]: what the host planner needs of every new packet.
template <int HS>
VBMD_HD void vbml_walk_entry(const vbml_arrays &A, const int *bs, const vbml_plan &p, const long long *src_off,
                             const int *head_status, const int *head_W, const long long *granulepos,
                             const uint8_t *eos, const uint8_t *gap, int *pk_status, long long *pk_out_end,
                             vbml_back &back)
{
    vbml_slot s = A.slots[p.sid];
    const long long P0 = (long long)p.sid * (A.MP + 1);
    if (p.status) {                                        // refused: the slot stays as it is
        for (int k = p.k0; k < p.k1; k++) {
            pk_status[k] = head_status[k];
            pk_out_end[k] = s.at;
        }
        const vbml_back b = {p.status, 0, s.count, 0, s.lo, s.at, A.offsets[P0 + s.count] - A.offsets[P0]};
        back = b;
        return;
    }
    if (p.drop > 0) {                                      // the first valid packet that is left
        s.hasv = 0;
        for (int t = 0; t < p.keep && !s.hasv; t++)
            if (A.status[P0 + t] == 0) {
                s.lo = A.out_start[P0 + t] + (A.end[P0 + t] - A.begin[P0 + t]);
                s.hasv = 1;
            }
    }
    const long long dst = A.offsets[P0 + p.keep], src0 = src_off[p.k0];
    int j = p.keep;
    for (int k = p.k0; k < p.k1; k++, j++) {
        if (gap && gap[k]) s.sc = s.gp = -1;               // packets were lost in front: k_run_plan's rule
        const int st = head_status[k];
        long b = 0, e = 0;
        if (st == 0) {
            const int W = head_W[k];
            vbmd_blockin<HS>(bs, s.lastW, W, granulepos ? granulepos[k] : -1, eos ? eos[k] : 0, s.sc, s.gp, b, e);
            s.lastW = W;
        }
        A.status[P0 + j] = st;
        A.begin[P0 + j] = (int)b;
        A.end[P0 + j] = (int)e;
        A.out_start[P0 + j] = s.at;
        A.offsets[P0 + j + 1] = dst + (src_off[k + 1] - src0);
        s.at += e - b;
        if (st == 0 && !s.hasv) {
            s.lo = s.at;
            s.hasv = 1;
        }
        pk_status[k] = st;
        pk_out_end[k] = s.at;
    }
    s.count = j;
    if (!s.hasv) s.lo = s.at;
    A.slots[p.sid] = s;
    const vbml_back b = {0, p.drop, j, p.by, s.lo, s.at, A.offsets[P0 + j] - A.offsets[P0]};
    back = b;
}

// The twin's append of one entry over host memory: the four steps in a row, the two moves as memmove and memcpy.  Pure
// host code over plain arrays: a stand-alone program can run it (tests/native/live_store_host.cpp).
template <int HS>
inline void vbml_host_append_entry(const vbml_arrays &A, const int *bs, int sid, int k0, int k1, const uint8_t *src,
                                   const long long *src_off, long long src_bytes, const int *head_status,
                                   const int *head_W, const long long *granulepos, const uint8_t *eos,
                                   const uint8_t *gap, int *pk_status, long long *pk_out_end, vbml_back &back)
{
    vbml_plan p;
    vbml_plan_entry(A, sid, k0, k1, src_off, src_bytes, p);
    const long long P0 = (long long)sid * (A.MP + 1);
    uint8_t *base = A.data + (long long)sid * A.stride;
    if (p.drop > 0 && p.keep > 0) {                        // k_live_compact's move
        for (int k = 0; k <= p.keep; k++) A.offsets[P0 + k] = A.offsets[P0 + p.drop + k] - p.cut;
        memmove(A.out_start + P0, A.out_start + P0 + p.drop, (size_t)p.keep * sizeof(long long));
        memmove(A.status + P0, A.status + P0 + p.drop, (size_t)p.keep * sizeof(int));
        memmove(A.begin + P0, A.begin + P0 + p.drop, (size_t)p.keep * sizeof(int));
        memmove(A.end + P0, A.end + P0 + p.drop, (size_t)p.keep * sizeof(int));
        memmove(base, base + p.cut, (size_t)p.kept);
    }
    vbml_walk_entry<HS>(A, bs, p, src_off, head_status, head_W, granulepos, eos, gap, pk_status, pk_out_end, back);
    const long long nb = p.status ? 0 : src_off[k1] - src_off[k0];
    if (nb > 0) memcpy(base + p.kept, src + src_off[k0], (size_t)nb);      // k_live_copy's
}

// ---- launches (live_store.hip) -----------------------------------------------------------------------------------------
#if defined(__HIPCC__) || defined(__HIP__)
struct vbmd_class;
// Entries [0, n) of an append, behind the head (k_index_head) over the caller's CSR.  d_tab: the entries' first packets
// [n + 1], in a mixed store their classes [n], then their slots [n] at d_tab + ids_at.  d_trimmed [n + 1]: workspace.
// bs_setup: the decoder's setup (null in a mixed store, whose slots take their block sizes from table[slot class]).
int vbml_launch_append(const vbml_arrays &A, int halfrate, const vbmd_setup *bs_setup, const vbmd_class *table, int n,
                       const int *d_tab, int ids_at, const uint8_t *d_src, const long long *d_src_off,
                       long long src_bytes, const int *d_head_status, const int *d_head_W,
                       const long long *d_granulepos, const uint8_t *d_eos, const uint8_t *d_gap, vbml_plan *d_plans,
                       int *d_trimmed, int *d_pk_status, long long *d_pk_out_end, vbml_back *d_back, hipStream_t q);
// slots d_ids[0 .. n) made fresh, of class d_cls[k] (null: the class they have)
int vbml_launch_restart(const vbml_arrays &A, int n, const int *d_ids, const int *d_cls, hipStream_t q);
#endif
