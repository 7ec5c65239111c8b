// Incremental Ogg demux on the device for many live streams (rules, state and workspace: ogg_feed.h; page rules and
// device helpers: ogg_demux.h), its host twin, and the C ABI over both (include/vorbis_mi355x.h, "Ogg demux, incremental
// form"; host scaffold: twin_host.h).
//
//   scan:  k_feed_gather      one wavefront per listed stream: carried page tail, then the chunk -> the stream's run in
//                             the work buffer
//          k_feed_walk        one lane per listed stream: resumes from the slot's state, takes whole pages
//                             (oggdmx_walk_step), stops at the first that is not whole; every read is bounded by the
//                             run's end
//          k_feed_scan_pages  one block, four entries per thread: exclusive scan of the page counts -> dense page numbers
//          k_feed_crc         one wavefront per page, as k_dmx_crc; records the first bad page of a stream
//          k_feed_settle      one lane per listed stream: a stream with a bad page is walked again up to it
//          k_feed_scan_counts one block: exclusive scans of packets and payload bytes; the totals
//          k_feed_info        one lane per listed stream: the bases into its call record, its info struct
//   fill:  k_feed_fill        one wavefront per page: packet ends and the payload part of the body, as k_dmx_fill; then
//                             one wavefront per stream: the carried part of its open packet to the front of its payload
//          k_feed_commit      one wavefront per page: header bytes and the open packet's bytes to the slot's stores; then
//                             one wavefront per stream: the unconsumed tail and the new state
//          k_feed_mark        the scan is committed
//   reset: k_feed_reset       one lane per listed stream: the slot's state back to all zero
// A resync feed (vbm_ogg_feed_create2 with VBM_OGG_FEED_RESYNC) runs one kernel in the place of walk, crc and settle:
//          k_feed_resync_walk one wavefront per listed stream (oggfeed_rs_walk with FeedWaveOps): the capture search
//                             tests one 4-byte window per lane over 64 positions and a ballot finds the first hit; per
//                             candidate every lane loads one header byte and four lacing bytes, a wave reduction gives
//                             the body length, and the CRC is dmx_wave_page_crc at once, because it decides where the
//                             walk goes next
//          k_feed_events      one lane per listed stream: its event struct
// A multiplexed feed (VBM_OGG_FEED_MULTIPLEXED) runs the <true> forms of k_feed_walk, k_feed_settle and
// k_feed_resync_walk: the same walks with the group rule of ogg_feed.h in front of every page.  The strict walk reads a
// head page's 7 mark bytes plainly; the wave walk takes them out of the dwords its `head` op has already loaded.  The
// other feeds run the <false> forms, in which no statement of the rule is left.
// Nothing of a slot changes before k_feed_commit, which runs only after a fill that wrote its outputs.
#include <hip/hip_runtime.h>
#include <string.h>
#include <new>
#include <string>
#include <vector>

#include "ogg_feed.h"
#include "twin_host.h"

namespace {

constexpr int kWaveBlocks = 2048;  // most blocks (of four wavefronts) a wave-parallel kernel is launched with
constexpr int kPiece = 1 << 30;    // dmx_wave_copy takes an int

struct FeedArgs {                  // the call's arguments in device (or host) memory
    const long long *off;          // [n + 1]
    const int *ids, *end;          // [n]
};

struct FeedMem {                   // the feed's state and workspace
    OggFeedState *state;
    uint8_t *tail, *open, *hdr, *work;
    OggDmxPage *pages;
    OggFeedCall *call;
    long long *npages, *page_base, *totals;
    long long *count, *base;       // [2 * max_streams]: packets and payload bytes of the call per listed stream, their sums
    int *bad, *status, *committed;
    OggFeedLink *link;             // resync feeds only (else null): [max_streams] the slots' links,
    OggFeedRsCall *rs;             // [max_streams] the listed streams of the scan beside `call`
    OggFeedMux *mux, *mux_next;    // multiplexed feeds only (else null): [max_streams] the slots' groups, and those of
                                   // the listed streams once the scan is committed
};

VBMX_HD long long feed_at(const long long *off, int i, const OggFeedCaps &caps)
{
    return off[i] - off[0] + (long long)i * caps.max_page_carry;
}

VBMX_HD long long feed_first_rec(const long long *off, int i) { return (off[i] - off[0]) / 27 + i; }

// stream i of the list, walked from its slot's state over its run in the work buffer
template <bool MUX>
VBMX_HD void feed_walk_one(const FeedArgs &a, const FeedMem &m, const OggFeedCaps &caps, int i, int limit, bool bad_at_limit,
                           OggFeedCall &c)
{
    const int slot = a.ids[i];
    const OggFeedState st = m.state[slot];
    const long long at = feed_at(a.off, i, caps), rec = feed_first_rec(a.off, i);
    const long long run_end = at + oggfeed_tail_in(st, caps) + (a.off[i + 1] - a.off[i]);
    OggFeedMux mx = {};
    if (MUX) mx = m.mux[slot];
    oggfeed_walk<MUX>(m.work, at, run_end, st, caps, a.end[i], limit, bad_at_limit, m.pages + rec,
                      feed_first_rec(a.off, i + 1) - rec, slot, c, mx);
    if (MUX) m.mux_next[i] = mx;
}

// ---- kernels ---------------------------------------------------------------------------------------------------

__device__ __forceinline__ void feed_wave_copy(uint8_t *dst, const uint8_t *src, long long n, int lane)
{
    for (; n > 0; n -= kPiece, dst += kPiece, src += kPiece) dmx_wave_copy(dst, src, (int)(n < kPiece ? n : kPiece), lane);
}

__global__ void __launch_bounds__(256) k_feed_gather(int n, FeedArgs a, FeedMem m, OggFeedCaps caps, const uint8_t *data)
{
    const int lane = threadIdx.x & 63, nwaves = gridDim.x * 4;
    for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += nwaves) {
        const int slot = a.ids[i];
        const OggFeedState st = m.state[slot];
        if (st.status || st.done) continue;
        const int tail = oggfeed_tail_in(st, caps);                // at most max_page_carry: never past the slot's store
        uint8_t *run = m.work + feed_at(a.off, i, caps);
        dmx_wave_copy(run, m.tail + (long long)slot * caps.max_page_carry, tail, lane);
        feed_wave_copy(run + tail, data + a.off[i], a.off[i + 1] - a.off[i], lane);
    }
}

template <bool MUX>
__global__ void __launch_bounds__(64) k_feed_walk(int n, FeedArgs a, FeedMem m, OggFeedCaps caps)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    OggFeedCall c;
    feed_walk_one<MUX>(a, m, caps, i, INT_MAX, false, c);
    m.call[i] = c;
    m.npages[i] = c.npages;
    m.count[2 * i] = c.packets, m.count[2 * i + 1] = c.payload_bytes;
    m.bad[i] = INT_MAX;
}

// oggfeed_rs_walk's four by the 64 lanes of a wavefront; every result is the same in every lane
struct FeedWaveOps {
    const uint32_t *T;             // the CRC table in LDS
    const OggMuxPow *pw;
    int lane;

    __device__ long long find(const uint8_t *work, long long pos, long long end) const
    {
        for (; pos + 4 <= end; pos += 64) {
            const long long p = pos + lane;
            const bool hit = p + 4 <= end && oggfeed_rs_capture(dmx_load4(work + p, 4));
            const unsigned long long hits = __ballot(hit);
            if (hits) return pos + __builtin_ctzll(hits);
        }
        return -1;
    }

    __device__ int head(const uint8_t *h, long long left, OggFeedHead &hd) const
    {
        // the round trip: header byte `lane`, and lacing values 4 * lane .. 4 * lane + 3 if the run goes on that far
        // (past nseg they are body bytes of this run, and are masked below)
        const int hb = lane < 27 && lane < left ? h[lane] : 0;
        const uint32_t lw = dmx_load4(h + 27 + 4 * lane, left - 27 - 4 * lane);
        if (left >= 5 && __builtin_amdgcn_readlane(hb, 4) != 0) return 0;
        if (left < 27) return -2;
        hd.flags = __builtin_amdgcn_readlane(hb, 5), hd.nseg = __builtin_amdgcn_readlane(hb, 26);
        hd.serial = field(hb, 14), hd.seq = field(hb, 18);
        if (left - 27 < hd.nseg) return -2;
        const int mine = min(4, max(0, hd.nseg - 4 * lane));       // how many of my four are lacing values
        const uint32_t v = mine == 4 ? lw : lw & ((1u << (8 * mine)) - 1u);
        int body = (int)((v & 0xff) + ((v >> 8) & 0xff) + ((v >> 16) & 0xff) + (v >> 24));
        for (int m = 32; m >= 1; m >>= 1) body += __shfl_xor(body, m, 64);
        hd.body = __builtin_amdgcn_readfirstlane(body);
        hd.lace = lw;
        return left - 27 - hd.nseg < hd.body ? -2 : 1;
    }

    // The page is whole and its body has 7 bytes or more.  They begin at byte nseg of the 256 that `head` loaded, four
    // to a lane: with 244 segments or fewer, bytes nseg .. nseg + 7 lie in the dwords of lanes nseg / 4 .. nseg / 4 + 2
    // (62 at most; the eighth byte, which may lie behind the run and then reads as 0, is masked by oggsel_is_mark).  A
    // head page of more segments takes a second round trip: 7 byte reads at the same address in every lane.
    __device__ bool mark(const uint8_t *h, const OggFeedHead &hd) const
    {
        uint32_t lo, hi;
        if (hd.nseg <= 244) {
            const int d = hd.nseg >> 2, sh = (hd.nseg & 3) * 8;
            const uint64_t w0 = (uint32_t)__builtin_amdgcn_readlane((int)hd.lace, d);
            const uint64_t w1 = (uint32_t)__builtin_amdgcn_readlane((int)hd.lace, d + 1);
            const uint64_t w2 = (uint32_t)__builtin_amdgcn_readlane((int)hd.lace, d + 2);
            lo = (uint32_t)((w0 | (w1 << 32)) >> sh);
            hi = (uint32_t)((w1 | (w2 << 32)) >> sh);
        } else {
            const uint8_t *b = h + 27 + hd.nseg;
            lo = dmx_load4(b, 4);
            hi = dmx_load4(b + 4, 3);
        }
        return oggsel_is_mark(lo, hi);
    }

    __device__ bool crc(const uint8_t *h, int len) const
    {
        return __builtin_amdgcn_readfirstlane((int)dmx_wave_page_crc(T, *pw, h, len, lane)) != 0;
    }

    // header bytes at .. at + 3, each in its lane, as one word
    static __device__ uint32_t field(int hb, int at)
    {
        return (uint32_t)__builtin_amdgcn_readlane(hb, at) | ((uint32_t)__builtin_amdgcn_readlane(hb, at + 1) << 8) |
               ((uint32_t)__builtin_amdgcn_readlane(hb, at + 2) << 16) | ((uint32_t)__builtin_amdgcn_readlane(hb, at + 3) << 24);
    }
};

// stream i of the list by the rules of the resync mode; writer: this caller stores the group state (the device walk
// holds it in every lane)
template <bool MUX, class Ops>
VBMX_HD void feed_rs_walk_one(const Ops &ops, const FeedArgs &a, const FeedMem &m, const OggFeedCaps &caps, int i,
                              OggFeedCall &c, OggFeedRsCall &r, bool writer)
{
    const int slot = a.ids[i];
    const OggFeedState st = m.state[slot];
    const long long at = feed_at(a.off, i, caps), rec = feed_first_rec(a.off, i);
    const int tail_in = oggfeed_tail_in(st, caps);
    OggFeedMux mx = {};
    if (MUX) mx = m.mux[slot];
    oggfeed_rs_walk<MUX>(ops, m.work, at, at + tail_in + (a.off[i + 1] - a.off[i]), tail_in, st, m.link[slot], caps,
                         a.end[i], m.pages + rec, feed_first_rec(a.off, i + 1) - rec, slot, c, r, mx);
    if (MUX && writer) m.mux_next[i] = mx;
}

template <bool MUX>
__global__ void __launch_bounds__(256) k_feed_resync_walk(int n, OggMuxPow pw, FeedArgs a, FeedMem m, OggFeedCaps caps)
{
    __shared__ uint32_t T[256];
    T[threadIdx.x] = oggmux_crc_entry(threadIdx.x);
    __syncthreads();
    const int lane = threadIdx.x & 63, nwaves = gridDim.x * 4;
    const FeedWaveOps ops = {T, &pw, lane};
    // the wavefront's number, as a scalar: the slot's state and every count of the walk stay in scalar registers
    for (int i = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)); i < n; i += nwaves) {
        OggFeedCall c;
        OggFeedRsCall r;
        feed_rs_walk_one<MUX>(ops, a, m, caps, i, c, r, lane == 0);
        if (lane == 0) {
            m.call[i] = c;
            m.rs[i] = r;
            m.npages[i] = c.npages;
            m.count[2 * i] = c.packets, m.count[2 * i + 1] = c.payload_bytes;
        }
    }
}

__global__ void __launch_bounds__(256) k_feed_events(int n, const OggFeedRsCall *rs, vbm_ogg_feed_events *out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = rs[i].ev;
}

__global__ void __launch_bounds__(256) k_feed_scan_pages(int n, const long long *npages, long long *page_base)
{
    __shared__ long long wave_sum[4];
    block_scan_array<1>(n, npages, page_base, page_base + n, wave_sum);
}

__global__ void __launch_bounds__(256) k_feed_crc(int n, OggMuxPow pw, FeedArgs a, FeedMem m)
{
    __shared__ uint32_t T[256];
    T[threadIdx.x] = oggmux_crc_entry(threadIdx.x);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const long long total = m.page_base[n], nwaves = (long long)gridDim.x * 4;
    for (long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); p < total; p += nwaves) {
        long long k;
        const int i = oggdmx_entry_of_page(m.page_base, n, p, k);
        const OggDmxPage pg = m.pages[feed_first_rec(a.off, i) + k];
        const bool ok = dmx_wave_page_crc(T, pw, m.work + pg.at, pg.len, lane);
        if (lane == 0 && !ok) atomicMin(&m.bad[i], (int)k);
    }
}

template <bool MUX>
__global__ void __launch_bounds__(64) k_feed_settle(int n, FeedArgs a, FeedMem m, OggFeedCaps caps)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const int bad = m.bad[i];
    if (bad >= m.npages[i]) return;
    OggFeedCall c;                                  // pages from the bad one on are not taken
    feed_walk_one<MUX>(a, m, caps, i, bad, true, c);
    m.call[i] = c;
    m.count[2 * i] = c.packets, m.count[2 * i + 1] = c.payload_bytes;
}

__global__ void __launch_bounds__(256) k_feed_scan_counts(int n, FeedMem m, long long *out_totals)
{
    __shared__ long long wave_sum[4];
    block_scan_array<2>(n, m.count, m.base, m.totals, wave_sum);
    block_scan_array<2>(n, m.count + 1, m.base + 1, m.totals + 1, wave_sum);
    if (threadIdx.x == 0) {
        out_totals[0] = m.totals[0];
        out_totals[1] = m.totals[1];
        *m.committed = 0;
    }
}

__global__ void __launch_bounds__(256) k_feed_info(int n, FeedMem m, vbm_ogg_feed_info *out_info)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    m.call[i].packet_base = m.base[2 * i];
    m.call[i].payload_base = m.base[2 * i + 1];
    vbm_ogg_feed_info fi;
    if (m.rs) oggfeed_rs_info(m.call[i], m.rs[i], fi);
    else oggfeed_info(m.call[i], fi);
    out_info[i] = fi;
}

// gap: null, or one mark per packet: the first packet of an entry whose scan met a gap gets 1, every other 0
__global__ void __launch_bounds__(256) k_feed_fill(int n, FeedArgs a, FeedMem m, OggFeedCaps caps, long long packet_cap,
                                                   long long payload_cap, OggDmxOut out, uint8_t *gap)
{
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (*m.committed) {                             // a fill has already written and committed this scan
        if (first) *m.status = VBM_EINVAL;
        return;
    }
    if (m.totals[0] > packet_cap || m.totals[1] > payload_cap) {
        if (first) *m.status = VBM_OGG_DEMUX_ECAP;  // the call does not fit: nothing is written, nothing committed
        return;
    }
    if (first) {
        *m.status = 0;
        out.offsets[0] = 0;
    }
    const int lane = threadIdx.x & 63, wave = blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long total = m.page_base[n], nwaves = (long long)gridDim.x * 4;
    for (long long p = wave; p < total; p += nwaves) {
        long long k;
        const int i = oggdmx_entry_of_page(m.page_base, n, p, k);
        const OggFeedCall &c = m.call[i];
        if (k >= c.npages) continue;                // behind a page whose CRC failed
        OggDmxPageCtx x;
        oggfeed_ctx_payload(m.work, m.pages[feed_first_rec(a.off, i) + k], c, x);
        dmx_wave_packet_ends(x, out, lane);
        const OggDmxSplit s = oggdmx_body_split(x, out);
        if (s.n_p) dmx_wave_copy(s.dst_p, s.src_p, (int)s.n_p, lane);
    }
    for (long long i = wave; i < n; i += nwaves) {
        const OggFeedCall &c = m.call[i];
        const int open_in = min(c.open_in, caps.max_packet_bytes);   // never past the slot's store
        if (open_in > 0)
            dmx_wave_copy(out.payload + c.payload_base, m.open + (long long)c.slot * caps.max_packet_bytes, open_in, lane);
        if (gap) {
            const int mark = m.rs ? m.rs[i].ev.gaps : 0;
            for (long long k = lane; k < c.packets; k += 64) gap[c.packet_base + k] = k == 0 && mark;
        }
    }
}

__global__ void __launch_bounds__(256) k_feed_commit(int n, FeedArgs a, FeedMem m, OggFeedCaps caps)
{
    if (*m.status != 0) return;                     // the fill wrote nothing
    const OggDmxOut keep = {m.hdr, m.open, nullptr, nullptr, nullptr};
    const int lane = threadIdx.x & 63, wave = blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long total = m.page_base[n], nwaves = (long long)gridDim.x * 4;
    for (long long p = wave; p < total; p += nwaves) {
        long long k;
        const int i = oggdmx_entry_of_page(m.page_base, n, p, k);
        const OggFeedCall &c = m.call[i];
        if (k >= c.npages) continue;
        OggDmxPageCtx xh, xo;
        oggfeed_ctx_keep(m.work, m.pages[feed_first_rec(a.off, i) + k], c, caps, xh, xo);
        const OggDmxSplit sh = oggdmx_body_split(xh, keep), so = oggdmx_body_split(xo, keep);
        if (sh.n_h) dmx_wave_copy(sh.dst_h, sh.src_h, (int)sh.n_h, lane);
        if (so.n_p) dmx_wave_copy(so.dst_p, so.src_p, (int)so.n_p, lane);
    }
    for (long long i = wave; i < n; i += nwaves) {
        const OggFeedCall &c = m.call[i];
        const int tail = c.next.tail;
        if (tail > 0 && tail <= caps.max_page_carry)
            dmx_wave_copy(m.tail + (long long)c.slot * caps.max_page_carry, m.work + c.pos_end, tail, lane);
        if (lane == 0) m.state[c.slot] = c.next;
        if (lane == 0 && m.rs) m.link[c.slot] = m.rs[i].next;
        if (lane == 0 && m.mux) m.mux[c.slot] = m.mux_next[i];
    }
}

__global__ void k_feed_mark(FeedMem m)
{
    if (*m.status == 0) *m.committed = 1;
}

__global__ void __launch_bounds__(256) k_feed_reset(int n, const int *ids, OggFeedState *state, OggFeedLink *link,
                                                    OggFeedMux *mux)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    state[ids[i]] = OggFeedState{};
    if (link) link[ids[i]] = OggFeedLink{};
    if (mux) mux[ids[i]] = OggFeedMux{};
}

}  // namespace

// ---- host side (scaffold: twin_host.h) --------------------------------------------------------------------------

struct vbm_ogg_feed {
    bool host = false, resync = false, mux = false;
    int max_streams = 0;
    long long max_call_bytes = 0;
    OggFeedCaps caps = {};
    OggMuxPow pow;
    TwinMem mem;                         // owns what m and args point to
    FeedMem m = {};
    uint8_t *args = nullptr;             // the call's arguments: off [n + 1], ids [n], end [n]; room for n = max_streams
    ArgStage stage;                      // device feed: they go up through it; the size of args
    std::vector<int> seen;               // [max_streams] the call that last listed a slot
    int call_no = 0;
    // the last scan
    bool scanned = false, host_committed = false;
    int n = 0;
    long long span = 0;
};

namespace {

size_t args_bytes(int n) { return ((size_t)n + 1) * sizeof(long long) + 2 * (size_t)n * sizeof(int); }

FeedArgs args_view(uint8_t *base, int n)
{
    FeedArgs a;
    a.off = (const long long *)base;
    a.ids = (const int *)(base + ((size_t)n + 1) * sizeof(long long));
    a.end = a.ids + n;
    return a;
}

int create(vbm_ogg_feed **out, int max_streams, long long max_call_bytes, int max_page_carry, int max_packet_bytes,
           int header_cap, unsigned flags, bool host, const char *name)
{
    if (!out || max_streams < 1 || max_call_bytes < 0 || max_page_carry < 1 || max_page_carry > 65307 ||
        max_packet_bytes < 1 || header_cap < 1 || (flags & ~(VBM_OGG_FEED_RESYNC | VBM_OGG_FEED_MULTIPLEXED)))
        return fail(VBM_EINVAL, std::string(name) + ": bad argument (max_streams >= 1, max_call_bytes >= 0, max_page_carry "
                                                    "in 1..65307, max_packet_bytes >= 1, header_cap >= 1, flags of "
                                                    "VBM_OGG_FEED_RESYNC | VBM_OGG_FEED_MULTIPLEXED)");
    if (!host) {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n < 1) return fail(VBM_ENODEV, "vbm_ogg_feed_create: no HIP device");
    }
    vbm_ogg_feed *f = new (std::nothrow) vbm_ogg_feed();
    if (!f) return fail(VBM_EFAULT, "vbm_ogg_feed_create: out of memory");
    f->host = f->mem.host = host;
    f->resync = (flags & VBM_OGG_FEED_RESYNC) != 0;
    f->mux = (flags & VBM_OGG_FEED_MULTIPLEXED) != 0;
    f->max_streams = max_streams;
    f->max_call_bytes = max_call_bytes;
    f->caps = {max_page_carry, max_packet_bytes, header_cap};
    f->pow = oggmux_pow_table();
    const size_t S = (size_t)max_streams;
    const char *who = "vbm_ogg_feed";
    int rc = VBM_OK;
    try {
        f->seen.assign(S, 0);
    } catch (const std::bad_alloc &) {
        rc = fail(VBM_EFAULT, "vbm_ogg_feed_create: out of memory");
    }
    if (!rc) rc = f->mem.get(f->m.state, S, who);
    if (!rc) rc = f->mem.get(f->m.tail, S * (size_t)max_page_carry, who);
    if (!rc) rc = f->mem.get(f->m.open, S * (size_t)max_packet_bytes, who);
    if (!rc) rc = f->mem.get(f->m.hdr, S * (size_t)header_cap, who);
    if (!rc) rc = f->mem.get(f->m.work, (size_t)max_call_bytes + S * (size_t)max_page_carry + 4, who);
    if (!rc) rc = f->mem.get(f->m.pages, (size_t)(max_call_bytes / 27) + S + 1, who);
    if (!rc) rc = f->mem.get(f->m.call, S, who);
    if (!rc) rc = f->mem.get(f->m.npages, S, who);
    if (!rc) rc = f->mem.get(f->m.page_base, S + 1, who);
    if (!rc) rc = f->mem.get(f->m.totals, 2, who);
    if (!rc) rc = f->mem.get(f->m.count, 2 * S, who);
    if (!rc) rc = f->mem.get(f->m.base, 2 * S, who);
    if (!rc) rc = f->mem.get(f->m.bad, S, who);
    if (!rc) rc = f->mem.get(f->m.status, 1, who);
    if (!rc) rc = f->mem.get(f->m.committed, 1, who);
    if (!rc) rc = f->mem.get(f->args, args_bytes(max_streams), who);
    if (!rc && f->resync) rc = f->mem.get(f->m.link, S, who);
    if (!rc && f->resync) rc = f->mem.get(f->m.rs, S, who);
    if (!rc && f->mux) rc = f->mem.get(f->m.mux, S, who);
    if (!rc && f->mux) rc = f->mem.get(f->m.mux_next, S, who);
    if (!rc && !host) rc = f->stage.create(args_bytes(max_streams), "vbm_ogg_feed_create: staging");
    if (rc) {
        vbm_ogg_feed_destroy(f);
        return rc;
    }
    *out = f;
    return VBM_OK;
}

// ids: each in range, none twice (f->seen is marked: call once per call, after every other check)
int check_ids(vbm_ogg_feed *f, int n, const int *ids, const char *who)
{
    if (n < 0 || n > f->max_streams) return fail(VBM_EINVAL, std::string(who) + ": n is negative or above max_streams");
    if (n && !ids) return fail(VBM_EINVAL, std::string(who) + ": null pointer");
    for (int i = 0; i < n; i++)
        if (ids[i] < 0 || ids[i] >= f->max_streams)
            return fail(VBM_EINVAL, std::string(who) + ": stream id " + std::to_string(ids[i]) + " is out of range");
    if (++f->call_no == INT_MAX) {
        f->seen.assign(f->seen.size(), 0);
        f->call_no = 1;
    }
    for (int i = 0; i < n; i++) {
        if (f->seen[ids[i]] == f->call_no)
            return fail(VBM_EINVAL, std::string(who) + ": stream id " + std::to_string(ids[i]) + " is listed twice");
        f->seen[ids[i]] = f->call_no;
    }
    return VBM_OK;
}

int check_scan(vbm_ogg_feed *f, bool host, int n, const int *ids, const uint8_t *data, const long long *off,
               const vbm_ogg_feed_info *info, const long long *totals, const char *who)
{
    int rc = check_kind(f, host, who, "feed");
    if (rc) return rc;
    if (n < 0 || n > f->max_streams) return fail(VBM_EINVAL, std::string(who) + ": n is negative or above max_streams");
    if (!off || !totals || (n && (!info || !ids))) return fail(VBM_EINVAL, std::string(who) + ": null pointer");
    if (off[0] < 0) return fail(VBM_EINVAL, std::string(who) + ": negative chunk offset");
    for (int i = 0; i < n; i++)
        if (off[i + 1] < off[i]) return fail(VBM_EINVAL, std::string(who) + ": chunk offsets decrease");
    if (off[n] - off[0] > f->max_call_bytes)
        return fail(VBM_EINVAL, std::string(who) + ": the chunks span " + std::to_string(off[n] - off[0]) +
                                    " bytes, above max_call_bytes = " + std::to_string(f->max_call_bytes));
    if (off[n] > off[0] && !data) return fail(VBM_EINVAL, std::string(who) + ": null data");
    return check_ids(f, n, ids, who);
}

int check_events(const vbm_ogg_feed *f, bool host, const vbm_ogg_feed_events *events, const char *who)
{
    int rc = check_kind(f, host, who, "feed");
    if (rc) return rc;
    if (!f->resync) return fail(VBM_EINVAL, std::string(who) + ": needs a feed made with VBM_OGG_FEED_RESYNC");
    if (!f->scanned) return fail(VBM_EINVAL, std::string(who) + ": no scan has been made on this feed");
    if (f->n && !events) return fail(VBM_EINVAL, std::string(who) + ": null pointer");
    return VBM_OK;
}

int check_fill(const vbm_ogg_feed *f, bool host, const uint8_t *payload, long long payload_cap, const long long *offsets,
               const long long *granulepos, const uint8_t *eos, long long packet_cap, const char *who)
{
    int rc = check_kind(f, host, who, "feed");
    if (rc) return rc;
    if (!f->scanned) return fail(VBM_EINVAL, std::string(who) + ": no scan has been made on this feed");
    if (payload_cap < 0 || packet_cap < 0) return fail(VBM_EINVAL, std::string(who) + ": negative capacity");
    if (!offsets || (payload_cap && !payload) || (packet_cap && (!granulepos || !eos)))
        return fail(VBM_EINVAL, std::string(who) + ": null pointer");
    return VBM_OK;
}

// off [n + 1], ids [n] and end [n] (NULL: zeros) in the layout of args_view
void pack_args(uint8_t *dst, int n, const int *ids, const long long *off, const uint8_t *end)
{
    const FeedArgs a = args_view(dst, n);
    if (off) memcpy((void *)a.off, off, ((size_t)n + 1) * sizeof(long long));
    if (n) memcpy((void *)a.ids, ids, (size_t)n * sizeof(int));
    int *e = (int *)a.end;
    for (int i = 0; i < n; i++) e[i] = end ? (end[i] != 0) : 0;
}

// the call's arguments go up through a pinned slot; the only wait is for the copy out of it two calls ago
int upload_args(vbm_ogg_feed *f, int n, const int *ids, const long long *off, const uint8_t *end, hipStream_t q,
                const char *who)
{
    void *h_args;
    const int rc = f->stage.next(h_args, who);
    if (rc) return rc;
    pack_args((uint8_t *)h_args, n, ids, off, end);
    // one copy: the three arrays lie in one block, in the same layout on both sides
    return f->stage.send(f->args, args_bytes(n), q, who);
}

dim3 wave_grid(long long waves)
{
    const long long blocks = (waves + 3) / 4;
    return dim3((unsigned)(blocks < 1 ? 1 : (blocks < kWaveBlocks ? blocks : kWaveBlocks)));
}

// pages of a call: every stream's first page and then one per 27 bytes at the very most; far fewer in practice, and the
// kernels stride over what the grid does not cover
dim3 page_grid(const vbm_ogg_feed *f) { return wave_grid(f->n + f->span / 1024); }

}  // namespace

extern "C" int vbm_ogg_feed_create(vbm_ogg_feed **fd, int max_streams, long long max_call_bytes, int max_page_carry,
                                   int max_packet_bytes, int header_cap)
{
    return create(fd, max_streams, max_call_bytes, max_page_carry, max_packet_bytes, header_cap, 0, false, "vbm_ogg_feed_create");
}

extern "C" int vbm_host_ogg_feed_create(vbm_ogg_feed **fd, int max_streams, long long max_call_bytes, int max_page_carry,
                                        int max_packet_bytes, int header_cap)
{
    return create(fd, max_streams, max_call_bytes, max_page_carry, max_packet_bytes, header_cap, 0, true, "vbm_host_ogg_feed_create");
}

extern "C" int vbm_ogg_feed_create2(vbm_ogg_feed **fd, int max_streams, long long max_call_bytes, int max_page_carry,
                                    int max_packet_bytes, int header_cap, unsigned flags)
{
    return create(fd, max_streams, max_call_bytes, max_page_carry, max_packet_bytes, header_cap, flags, false, "vbm_ogg_feed_create2");
}

extern "C" int vbm_host_ogg_feed_create2(vbm_ogg_feed **fd, int max_streams, long long max_call_bytes, int max_page_carry,
                                         int max_packet_bytes, int header_cap, unsigned flags)
{
    return create(fd, max_streams, max_call_bytes, max_page_carry, max_packet_bytes, header_cap, flags, true, "vbm_host_ogg_feed_create2");
}

extern "C" void vbm_ogg_feed_destroy(vbm_ogg_feed *f)
{
    if (!f) return;
    f->mem.free_all();
    f->stage.destroy();
    delete f;
}

extern "C" int vbm_ogg_feed_scan(vbm_ogg_feed *f, int n, const int *ids, const uint8_t *d_data,
                                 const long long *chunk_offsets, const uint8_t *end, vbm_ogg_feed_info *d_info,
                                 long long *d_totals, void *stream)
{
    int rc = check_scan(f, false, n, ids, d_data, chunk_offsets, d_info, d_totals, "vbm_ogg_feed_scan");
    if (rc) return rc;
    hipStream_t q = (hipStream_t)stream;
    rc = upload_args(f, n, ids, chunk_offsets, end, q, "vbm_ogg_feed_scan: upload of the arguments");
    if (rc) return rc;
    f->scanned = true;
    f->n = n;
    f->span = chunk_offsets[n] - chunk_offsets[0];
    const FeedArgs a = args_view(f->args, n);
    if (n > 0) {
        hipLaunchKernelGGL(k_feed_gather, wave_grid(n), dim3(256), 0, q, n, a, f->m, f->caps, d_data);
        const auto rs_walk = f->mux ? k_feed_resync_walk<true> : k_feed_resync_walk<false>;
        const auto walk = f->mux ? k_feed_walk<true> : k_feed_walk<false>;
        if (f->resync) hipLaunchKernelGGL(rs_walk, wave_grid(n), dim3(256), 0, q, n, f->pow, a, f->m, f->caps);
        else hipLaunchKernelGGL(walk, dim3((n + 63) / 64), dim3(64), 0, q, n, a, f->m, f->caps);
    }
    hipLaunchKernelGGL(k_feed_scan_pages, dim3(1), dim3(256), 0, q, n, f->m.npages, f->m.page_base);
    if (n > 0 && !f->resync) {                      // a resync walk has judged every CRC itself
        hipLaunchKernelGGL(k_feed_crc, page_grid(f), dim3(256), 0, q, n, f->pow, a, f->m);
        const auto settle = f->mux ? k_feed_settle<true> : k_feed_settle<false>;
        hipLaunchKernelGGL(settle, dim3((n + 63) / 64), dim3(64), 0, q, n, a, f->m, f->caps);
    }
    hipLaunchKernelGGL(k_feed_scan_counts, dim3(1), dim3(256), 0, q, n, f->m, d_totals);
    if (n > 0) hipLaunchKernelGGL(k_feed_info, dim3((n + 255) / 256), dim3(256), 0, q, n, f->m, d_info);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? VBM_OK : vbm_set_hip_error(e, "vbm_ogg_feed_scan: launch");
}

extern "C" int vbm_ogg_feed_scan_events(vbm_ogg_feed *f, vbm_ogg_feed_events *d_events, void *stream)
{
    int rc = check_events(f, false, d_events, "vbm_ogg_feed_scan_events");
    if (rc || f->n == 0) return rc;
    hipLaunchKernelGGL(k_feed_events, dim3((f->n + 255) / 256), dim3(256), 0, (hipStream_t)stream, f->n, f->m.rs, d_events);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? VBM_OK : vbm_set_hip_error(e, "vbm_ogg_feed_scan_events: launch");
}

// vbm_ogg_feed_fill (d_gap null) and vbm_ogg_feed_fill_gaps
static int fill_device(vbm_ogg_feed *f, uint8_t *d_payload, long long payload_cap, long long *d_offsets,
                       long long *d_granulepos, uint8_t *d_eos, uint8_t *d_gap, long long packet_cap, void *stream,
                       const char *who)
{
    int rc = check_fill(f, false, d_payload, payload_cap, d_offsets, d_granulepos, d_eos, packet_cap, who);
    if (rc) return rc;
    hipStream_t q = (hipStream_t)stream;
    const FeedArgs a = args_view(f->args, f->n);
    // bases that are never written through (no header part here; no payload bytes when d_payload is null) stay non-null
    const OggDmxOut out = {f->m.hdr, d_payload ? d_payload : f->m.work, d_offsets, d_granulepos, d_eos};
    hipLaunchKernelGGL(k_feed_fill, page_grid(f), dim3(256), 0, q, f->n, a, f->m, f->caps, packet_cap, payload_cap, out,
                       d_gap);
    hipLaunchKernelGGL(k_feed_commit, page_grid(f), dim3(256), 0, q, f->n, a, f->m, f->caps);
    hipLaunchKernelGGL(k_feed_mark, dim3(1), dim3(1), 0, q, f->m);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? VBM_OK : vbm_set_hip_error(e, (std::string(who) + ": launch").c_str());
}

extern "C" int vbm_ogg_feed_fill(vbm_ogg_feed *f, uint8_t *d_payload, long long payload_cap, long long *d_offsets,
                                 long long *d_granulepos, uint8_t *d_eos, long long packet_cap, void *stream)
{
    return fill_device(f, d_payload, payload_cap, d_offsets, d_granulepos, d_eos, nullptr, packet_cap, stream,
                       "vbm_ogg_feed_fill");
}

extern "C" int vbm_ogg_feed_fill_gaps(vbm_ogg_feed *f, uint8_t *d_payload, long long payload_cap, long long *d_offsets,
                                      long long *d_granulepos, uint8_t *d_eos, uint8_t *d_gap, long long packet_cap,
                                      void *stream)
{
    return fill_device(f, d_payload, payload_cap, d_offsets, d_granulepos, d_eos, d_gap, packet_cap, stream,
                       "vbm_ogg_feed_fill_gaps");
}

extern "C" int vbm_ogg_feed_status(vbm_ogg_feed *f, int *status, void *stream)
{
    if (!f || !status) return fail(VBM_EINVAL, "vbm_ogg_feed_status: null pointer");
    return read_status(f->host, f->m.status, status, stream, "vbm_ogg_feed_status");
}

extern "C" int vbm_ogg_feed_headers(vbm_ogg_feed *f, int id, uint8_t *headers, long long cap, int *sizes, void *stream)
{
    if (!f || !sizes) return fail(VBM_EINVAL, "vbm_ogg_feed_headers: null pointer");
    if (id < 0 || id >= f->max_streams) return fail(VBM_EINVAL, "vbm_ogg_feed_headers: stream id out of range");
    hipStream_t q = (hipStream_t)stream;
    OggFeedState st;
    if (f->host) {
        st = f->m.state[id];
    } else {
        hipError_t e = hipMemcpyAsync(&st, f->m.state + id, sizeof(st), hipMemcpyDeviceToHost, q);
        if (e == hipSuccess) e = hipStreamSynchronize(q);
        if (e != hipSuccess) return vbm_set_hip_error(e, "vbm_ogg_feed_headers: state");
    }
    const OggDmxCounts &c = st.cnt;
    if (c.packets < 3 || c.h2 < 0 || c.h2 > f->caps.header_cap)
        return fail(VBM_EINVAL, "vbm_ogg_feed_headers: the stream has not completed its three header packets");
    sizes[0] = (int)c.h0, sizes[1] = (int)(c.h1 - c.h0), sizes[2] = (int)(c.h2 - c.h1);
    if (!headers) return VBM_OK;
    if (cap < c.h2) return fail(VBM_EINVAL, "vbm_ogg_feed_headers: cap is below the header packets' size");
    const uint8_t *src = f->m.hdr + (size_t)id * (size_t)f->caps.header_cap;
    if (f->host) {
        memcpy(headers, src, (size_t)c.h2);
        return VBM_OK;
    }
    hipError_t e = hipMemcpyAsync(headers, src, (size_t)c.h2, hipMemcpyDeviceToHost, q);
    if (e == hipSuccess) e = hipStreamSynchronize(q);
    return e == hipSuccess ? VBM_OK : vbm_set_hip_error(e, "vbm_ogg_feed_headers: copy");
}

extern "C" int vbm_ogg_feed_reset_streams(vbm_ogg_feed *f, int n, const int *ids, void *stream)
{
    if (!f) return fail(VBM_EINVAL, "vbm_ogg_feed_reset_streams: null pointer");
    int rc = check_ids(f, n, ids, "vbm_ogg_feed_reset_streams");
    if (rc) return rc;
    f->scanned = false;                             // a scan made before the reset is not filled after it
    if (f->host) {
        for (int i = 0; i < n; i++) {
            f->m.state[ids[i]] = OggFeedState{};
            if (f->resync) f->m.link[ids[i]] = OggFeedLink{};
            if (f->mux) f->m.mux[ids[i]] = OggFeedMux{};
        }
        return VBM_OK;
    }
    if (n == 0) return VBM_OK;
    hipStream_t q = (hipStream_t)stream;
    rc = upload_args(f, n, ids, nullptr, nullptr, q, "vbm_ogg_feed_reset_streams: upload of the ids");
    if (rc) return rc;
    hipLaunchKernelGGL(k_feed_reset, dim3((n + 255) / 256), dim3(256), 0, q, n, args_view(f->args, n).ids,
                       f->m.state, f->m.link, f->m.mux);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? VBM_OK : vbm_set_hip_error(e, "vbm_ogg_feed_reset_streams: launch");
}

// ---- the same on the CPU: the functions of ogg_feed.h and ogg_demux.h, stream after stream and page after page ------
extern "C" int vbm_host_ogg_feed_scan(vbm_ogg_feed *f, int n, const int *ids, const uint8_t *data,
                                      const long long *chunk_offsets, const uint8_t *end, vbm_ogg_feed_info *info,
                                      long long *totals)
{
    int rc = check_scan(f, true, n, ids, data, chunk_offsets, info, totals, "vbm_host_ogg_feed_scan");
    if (rc) return rc;
    const uint32_t *T = crc_table().t;
    pack_args(f->args, n, ids, chunk_offsets, end);
    f->scanned = true;
    f->host_committed = false;
    f->n = n;
    f->span = chunk_offsets[n] - chunk_offsets[0];
    const FeedArgs a = args_view(f->args, n);
    const FeedMem &m = f->m;
    long long npages = 0, packets = 0, payload = 0;
    for (int i = 0; i < n; i++) {
        const OggFeedState &st = m.state[ids[i]];
        if (!st.status && !st.done) {                              // gather
            const int tail = oggfeed_tail_in(st, f->caps);
            uint8_t *run = m.work + feed_at(a.off, i, f->caps);
            if (tail) memcpy(run, m.tail + (size_t)ids[i] * (size_t)f->caps.max_page_carry, (size_t)tail);
            if (a.off[i + 1] > a.off[i]) memcpy(run + tail, data + a.off[i], (size_t)(a.off[i + 1] - a.off[i]));
        }
        OggFeedCall c;
        const auto walk_one = f->mux ? feed_walk_one<true> : feed_walk_one<false>;
        if (f->resync) {
            const OggFeedSerialOps ops = {T, &f->pow};
            if (f->mux) feed_rs_walk_one<true>(ops, a, m, f->caps, i, c, m.rs[i], true);
            else feed_rs_walk_one<false>(ops, a, m, f->caps, i, c, m.rs[i], true);
        } else {
            walk_one(a, m, f->caps, i, INT_MAX, false, c);
            const OggDmxPage *pages = m.pages + feed_first_rec(a.off, i);
            for (int k = 0; k < c.npages; k++) {
                if (oggdmx_page_crc_ok(T, f->pow, m.work + pages[k].at, pages[k].len)) continue;
                walk_one(a, m, f->caps, i, k, true, c);            // pages from the bad one on are not taken
                break;
            }
        }
        c.packet_base = packets, c.payload_base = payload;
        packets += c.packets;
        payload += c.payload_bytes;
        m.page_base[i] = npages;
        npages += c.npages;
        m.call[i] = c;
        if (f->resync) oggfeed_rs_info(c, m.rs[i], info[i]);
        else oggfeed_info(c, info[i]);
    }
    m.page_base[n] = npages;
    m.totals[0] = totals[0] = packets;
    m.totals[1] = totals[1] = payload;
    return VBM_OK;
}

extern "C" int vbm_host_ogg_feed_scan_events(vbm_ogg_feed *f, vbm_ogg_feed_events *events)
{
    const int rc = check_events(f, true, events, "vbm_host_ogg_feed_scan_events");
    if (rc) return rc;
    for (int i = 0; i < f->n; i++) events[i] = f->m.rs[i].ev;
    return VBM_OK;
}

// vbm_host_ogg_feed_fill (gap null) and vbm_host_ogg_feed_fill_gaps
static int fill_host(vbm_ogg_feed *f, uint8_t *payload, long long payload_cap, long long *offsets, long long *granulepos,
                     uint8_t *eos, uint8_t *gap, long long packet_cap, const char *who)
{
    int rc = check_fill(f, true, payload, payload_cap, offsets, granulepos, eos, packet_cap, who);
    if (rc) return rc;
    const FeedMem &m = f->m;
    if (f->host_committed) {
        *m.status = VBM_EINVAL;
        return VBM_OK;
    }
    if (m.totals[0] > packet_cap || m.totals[1] > payload_cap) {
        *m.status = VBM_OGG_DEMUX_ECAP;
        return VBM_OK;
    }
    *m.status = 0;
    const FeedArgs a = args_view(f->args, f->n);
    // bases that are never written through (no header part here; no payload bytes when payload is null) stay non-null
    const OggDmxOut out = {m.hdr, payload ? payload : m.work, offsets, granulepos, eos};
    const OggDmxOut keep = {m.hdr, m.open, nullptr, nullptr, nullptr};
    offsets[0] = 0;
    for (int i = 0; i < f->n; i++) {
        const OggFeedCall &c = m.call[i];
        const OggDmxPage *pages = m.pages + feed_first_rec(a.off, i);
        const int open_in = c.open_in < f->caps.max_packet_bytes ? c.open_in : f->caps.max_packet_bytes;
        if (open_in > 0)
            memcpy(out.payload + c.payload_base, m.open + (size_t)c.slot * (size_t)f->caps.max_packet_bytes, (size_t)open_in);
        if (gap)
            for (long long k = 0; k < c.packets; k++) gap[c.packet_base + k] = k == 0 && f->resync && m.rs[i].ev.gaps;
        for (int k = 0; k < c.npages; k++) {
            OggDmxPageCtx x;
            oggfeed_ctx_payload(m.work, pages[k], c, x);
            oggdmx_page_packet_ends(x, out);
            const OggDmxSplit sp = oggdmx_body_split(x, out);
            if (sp.n_p) memcpy(sp.dst_p, sp.src_p, (size_t)sp.n_p);
        }
        // commit: after the stream's payload has been read out of its open store
        for (int k = 0; k < c.npages; k++) {
            OggDmxPageCtx xh, xo;
            oggfeed_ctx_keep(m.work, pages[k], c, f->caps, xh, xo);
            const OggDmxSplit sh = oggdmx_body_split(xh, keep), so = oggdmx_body_split(xo, keep);
            if (sh.n_h) memcpy(sh.dst_h, sh.src_h, (size_t)sh.n_h);
            if (so.n_p) memcpy(so.dst_p, so.src_p, (size_t)so.n_p);
        }
        const int tail = c.next.tail;
        if (tail > 0 && tail <= f->caps.max_page_carry)
            memcpy(m.tail + (size_t)c.slot * (size_t)f->caps.max_page_carry, m.work + c.pos_end, (size_t)tail);
        m.state[c.slot] = c.next;
        if (f->resync) m.link[c.slot] = m.rs[i].next;
        if (f->mux) m.mux[c.slot] = m.mux_next[i];
    }
    f->host_committed = true;
    return VBM_OK;
}

extern "C" int vbm_host_ogg_feed_fill(vbm_ogg_feed *f, uint8_t *payload, long long payload_cap, long long *offsets,
                                      long long *granulepos, uint8_t *eos, long long packet_cap)
{
    return fill_host(f, payload, payload_cap, offsets, granulepos, eos, nullptr, packet_cap, "vbm_host_ogg_feed_fill");
}

extern "C" int vbm_host_ogg_feed_fill_gaps(vbm_ogg_feed *f, uint8_t *payload, long long payload_cap, long long *offsets,
                                           long long *granulepos, uint8_t *eos, uint8_t *gap, long long packet_cap)
{
    return fill_host(f, payload, payload_cap, offsets, granulepos, eos, gap, packet_cap, "vbm_host_ogg_feed_fill_gaps");
}
