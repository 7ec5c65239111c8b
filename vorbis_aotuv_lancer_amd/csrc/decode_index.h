// The index of demuxed streams (status, [begin, end) and out_start of every packet, each stream's total), computed
// 64 packets at a time: written once for the device (k_index_scan, decode_index.hip: one wavefront per stream, a lane
// per packet) and for its host twin (vbm_host_decode_index_scan: the same code over arrays of 64 lanes).
//
// The rules are those of decode.h and are only called here: vbmd_head decides a packet's status and block size W,
// vbmd_blockin<HS> its [begin, end).  vbmd_index_stream (decode_setup.cpp) feeds vbmd_blockin the stream state one
// packet after the other; here every lane rebuilds the state in front of its own packet from prefix quantities over
// the valid packets (status 0), then calls vbmd_blockin itself:
//   lW        W of the last valid packet in front (a max-scan of lane numbers finds it), -1: none
//   sc        vbmd_blockin sets sc = 0 at the first valid packet and adds step = bs[lW]/4 + bs[W]/4 at every later
//             one, so sc in front of a packet is the sum of step over the valid packets after the first
//   gp        with j the last valid packet in front whose granulepos is not -1: granulepos[j] + (sc - sc after j),
//             since vbmd_blockin sets gp = granulepos[j] there and adds step at every packet without one; no j: -1
//   out_start the exclusive sum of end - begin
// vbmd_blockin reads gp == -1 as "none yet".  A granulepos below -1 can make the running gp land on -1 and un-set it,
// which no prefix sum expresses: a stream that holds a valid packet with granulepos < -1 is walked packet after packet
// (vbmi_serial) instead.  With every granulepos -1 or >= 0, gp stays >= 0 once set (step > 0) and the two agree.
#pragma once
#include "decode.h"

struct vbmi_state {          // a stream between two chunks of 64 packets
    int lastW;               // W of the last valid packet, -1: none yet
    int hasj;                // a valid packet with a granulepos has been seen: j
    long long sc;            // vbmd_blockin's sc after the last valid packet, -1: none yet
    long long jgp, jsc;      // granulepos[j], sc after j
    long long at;            // output samples so far
};

VBMD_HD vbmi_state vbmi_fresh()
{
    const vbmi_state st = {-1, 0, -1, 0, 0, 0};
    return st;
}

// Packet k of the CSR: vbmd_head's status; W = its block size flag (0 for a failed packet).  Offsets are clamped as
// vbmd_index_stream clamps them, so no byte outside [0, data_bytes) is read.
VBMD_HD int vbmi_head(const vbmd_setup &s, const uint8_t *data, const long long *offsets, long long data_bytes,
                      long long k, int &W)
{
    long long b = offsets[k], e = offsets[k + 1];
    b = b < 0 ? 0 : b > data_bytes ? data_bytes : b;
    e = e < b ? b : e > data_bytes ? data_bytes : e;
    vbmd_bits bits = {data + b, (long)(e - b), 0};
    int mode, lW, nW;
    W = 0;
    const int status = vbmd_head(s, bits, mode, W, lW, nW);
    if (status) W = 0;
    return status;
}

// The stream of packet k among streams [0, n): the largest i with first[i] <= k.  first [n + 1] does not decrease and
// first[0] <= k < first[n], so that stream is not empty and holds k.  This is how k_index_head<true> and the host twin
// (vbm_host_decode_index_scan_mixed) find the class of a packet: class[stream].
VBMD_HD int vbmi_stream_of(const int *first, int n, long long k)
{
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (first[mid] <= k) lo = mid;
        else hi = mid;
    }
    return lo;
}

// One stream, packet after packet from a fresh state, as vbmd_index_stream does it.  status [n] is given; begin [n]
// holds W on entry.
template <int HS>
VBMD_HD void vbmi_serial(const int *bs, long long n, const int *status, const long long *granulepos, const uint8_t *eos,
                         int *begin, int *end, long long *out_start, long long *out_end, long long *total)
{
    int lW = -1;
    long long sc = -1, gp = -1, at = 0;
    for (long long k = 0; k < n; k++) {
        long pb = 0, pe = 0;
        if (status[k] == 0) {
            const int W = begin[k];
            vbmd_blockin<HS>(bs, lW, W, granulepos ? granulepos[k] : -1, eos ? eos[k] : 0, sc, gp, pb, pe);
            lW = W;
        }
        begin[k] = (int)pb;
        end[k] = (int)pe;
        out_start[k] = at;
        at += pe - pb;
        if (out_end) out_end[k] = at;
    }
    *total = at;
}

// The next min(64, left) packets of a stream; every pointer is at the chunk's first packet, begin [] holds W on entry.
// Ops: the 64 lanes.  NL values of each per-lane quantity are held here (1 on the device, where the 64 lanes are the
// wavefront's; 64 on the host), lane(i) is the lane of value i, and
//   excl_max(v, out)    out = max of v over the lanes below, -1 for lane 0
//   incl_sum(v, out)    out = sum of v over the lanes up to and including this one
//   gather(v, idx, out) out = v of lane idx (idx < 0: any lane's)
//   last(st)            lane 63's st
template <class Ops, int HS>
VBMD_HD void vbmi_chunk(const int *bs, long long left, const int *status, const long long *granulepos,
                        const uint8_t *eos, int *begin, int *end, long long *out_start, long long *out_end,
                        vbmi_state &st)
{
    constexpr int NL = Ops::NL;
    int valid[NL], W[NL], eof[NL], k1[NL], k2[NL], p1[NL], p2[NL], Wp[NL], lW[NL], inc[NL], x[NL], xj[NL];
    int pb[NL], pe[NL], cnt[NL], y[NL];
    long long vgp[NL], gj[NL];
    for (int i = 0; i < NL; i++) {
        const int l = Ops::lane(i);
        valid[i] = l < left && status[l] == 0;
        W[i] = valid[i] ? begin[l] : 0;
        vgp[i] = valid[i] && granulepos ? granulepos[l] : -1;
        eof[i] = valid[i] && eos ? eos[l] : 0;
        k1[i] = valid[i] ? l : -1;
        k2[i] = valid[i] && vgp[i] != -1 ? l : -1;
    }
    Ops::excl_max(k1, p1);                       // the last valid packet in front, in this chunk
    Ops::excl_max(k2, p2);                       // ... that has a granulepos
    Ops::gather(W, p1, Wp);
    for (int i = 0; i < NL; i++) {
        lW[i] = p1[i] >= 0 ? Wp[i] : st.lastW;
        inc[i] = valid[i] && lW[i] >= 0 ? (bs[lW[i]] >> 2) + (bs[W[i]] >> 2) : 0;
    }
    Ops::incl_sum(inc, x);                       // a chunk adds at most 64 * blocksizes[1] / 2: an int holds it
    Ops::gather(x, p2, xj);
    Ops::gather(vgp, p2, gj);
    const long long base = st.sc < 0 ? 0 : st.sc;
    vbmi_state after[NL];
    for (int i = 0; i < NL; i++) {
        const long long sc_in = lW[i] < 0 ? -1 : base + (x[i] - inc[i]);
        const int hasj = p2[i] >= 0 || st.hasj;
        const long long jgp = p2[i] >= 0 ? gj[i] : st.jgp, jsc = p2[i] >= 0 ? base + xj[i] : st.jsc;
        long b = 0, e = 0;
        if (valid[i]) {
            long long sc = sc_in, gp = hasj ? jgp + (sc_in - jsc) : -1;
            vbmd_blockin<HS>(bs, lW[i], W[i], vgp[i], eof[i], sc, gp, b, e);
        }
        pb[i] = (int)b;
        pe[i] = (int)e;
        cnt[i] = (int)(e - b);
        vbmi_state &a = after[i];                // the stream's state behind this lane's packet
        a.lastW = valid[i] ? W[i] : lW[i];
        a.sc = a.lastW < 0 ? -1 : base + x[i];
        const bool isj = valid[i] && vgp[i] != -1;
        a.hasj = isj || hasj;
        a.jgp = isj ? vgp[i] : jgp;
        a.jsc = isj ? a.sc : jsc;
    }
    Ops::incl_sum(cnt, y);
    for (int i = 0; i < NL; i++) {
        const int l = Ops::lane(i);
        after[i].at = st.at + y[i];
        if (l < left) {
            begin[l] = pb[i];
            end[l] = pe[i];
            out_start[l] = st.at + (y[i] - cnt[i]);
            if (out_end) out_end[l] = st.at + y[i];
        }
    }
    st = Ops::last(after);
}

// ---- launches (decode_index.hip) -------------------------------------------------------------------------------------
#if defined(__HIPCC__) || defined(__HIP__)
struct vbmd_class;                   // decode_kernels.h
// status and W (into begin) of packets [0, P) of the CSR
int vbmd_launch_index_head(const vbmd_setup *d_setup, long long P, const uint8_t *d_data, const long long *d_offsets,
                           long long data_bytes, int *d_status, int *d_begin, hipStream_t q);
// the same for packets [d_first[0], d_first[nstreams]) of streams of a mixed decoder's classes: d_first [nstreams + 1],
// then the class of every stream [nstreams]; a packet takes the setup of its stream's class (vbmi_stream_of)
int vbmd_launch_index_head_mixed(const vbmd_class *table, int nstreams, const int *d_first, long long k0, long long k1,
                                 const uint8_t *d_data, const long long *d_offsets, long long data_bytes, int *d_status,
                                 int *d_begin, hipStream_t q);
// streams [0, nstreams): stream i is packets d_first[i] .. d_first[i + 1] of the arrays, whose begin [] holds W
// table: null, or the class table of a mixed decoder: stream i is then of class d_first[nstreams + 1 + i]
int vbmd_launch_index_scan(const vbmd_setup *d_setup, const vbmd_class *table, int halfrate, int nstreams,
                           const int *d_first, const int *d_status, const long long *d_granulepos, const uint8_t *d_eos, int *d_begin,
                           int *d_end, long long *d_out_start, long long *d_out_end, long long *d_totals, hipStream_t q);
#endif
