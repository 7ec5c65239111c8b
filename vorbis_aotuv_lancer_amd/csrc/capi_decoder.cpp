// C ABI of the batched device decoder (include/vorbis_mi355x.h, "decode" section).
//
// Every decode call enqueues, on the caller's stream: one table through the pinned staging ring (stage), then the front
// chain (enqueue_front): the clears, its own unpack kernel (entropy decode, row lists by block size), k_spectrum and
// one k_imdct launch per block size (each reads its row count from the device: rows of mixed block size are never
// sorted on the host); then its own overlap kernels.  Nothing waits on the device, except a staging slot that is still
// in flight from four turns back.
//   vbm_synthesis_batch: the row -> stream map, k_unpack, k_overlap.
//   vbm_synthesis_runs, whose rows are runs of consecutive packets of one stream: the run table (stream ids and run
//     starts), k_unpack_csr (from CSR offsets), k_run_plan, k_overlap_runs and k_run_commit.
//   vbm_synthesis_ranges, sample windows of the streams of a range store (packets and index in device memory): the host
//     plans pieces (a pre-roll packet and the packets after it) from the store's host index (range_plan.h, pure host
//     code); per sub-call the piece table, k_range_rows, k_unpack_rows, k_range_plan and k_overlap_runs.  No stream
//     state is read or written.
//
// vbm_range_store_create_device makes the store of vbm_range_store_create (check_csr and new_store serve both) from a
// CSR that is already in device memory, and vbm_decode_index_device the index alone: k_index_head and k_index_scan
// (decode_index.hip) in place of the host walk; the first packets of the streams go up through the staging ring.
//
// A half-rate decoder (vbm_decoder_create_halfrate) enqueues the same chains with the IMDCT of half each block size and
// the half-rate instantiations of the overlap kernels; its windows and trig tables are those of the halved sizes, its
// IMDCT rows, tails and PCM rows half as long.
//
// A mixed decoder (vbm_decoder_create_mixed) is the same object made from caps instead of a setup: its rows have
// max_channels channels and max_blocksize / 2 bins, it has a block list, a window and a trig table per block size the
// caps allow, and a table of classes (vbm_decoder_add_class) in place of the one setup.  vbm_synthesis_batch and
// vbm_synthesis_runs enqueue the same chains with the <MX = true> kernels: the class of every row goes up behind the
// ids or the run table in the same staging turn (from the host mirror of vbm_decoder_bind_streams' map), and there is
// one IMDCT launch per block size.  Fetch is refused on it.
//
// Range stores and the index of a mixed decoder (the _mixed creators, vbm_decode_index_device_mixed): the store keeps a
// host class column, one class per stream, which is its own and independent of vbm_decoder_bind_streams.
// vbm_synthesis_ranges sends the class of every piece (its stream's) behind the piece table in the same staging turn;
// k_range_rows spreads it over the piece's rows into the row-class column behind d_rows, and the rest of the chain is
// the <MX = true> one of vbm_synthesis_runs, its IMDCT grids sized by sum(rows x channels of the piece's class).  The
// index stages the streams' classes behind their first packets; k_index_head finds a packet's stream, hence class, by
// a search in that table, and k_index_scan takes stream i's block sizes from its class.
//
// Live range stores (vbm_live_store_*; rules, layout and kernels: live_store.h, live_store.hip): a range store with a
// fixed region per stream that takes appended runs (the arguments of vbm_synthesis_runs_gaps) and drops the oldest
// packets when a region is full.  An append enqueues k_index_head over the caller's CSR and the four live kernels, reads
// 40 B per entry and 12 B per new packet back and waits once; vbm_synthesis_ranges and vbm_ogg_cut_ranges read it
// through the view, which says where each stream's packets end and which sample is the first it still has.  The host
// twin (vbm_host_live_store_*) is the same object over host memory, with no decoder.
#include <algorithm>
#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "decode_index.h"
#include "decode_kernels.h"
#include "decode_setup.h"
#include "live_store.h"
#include "range_plan.h"
#include "vbm_internal.h"
#include "vorbis_mi355x.h"

extern "C" int vbm_host_mdct_trig(int n, float *out);

namespace {
constexpr int kStage = 4;
}

// set-up code: a HIP call that fails is recorded, and the function's own fail(rc) frees what it has made so far
#define CK(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) return fail(vbm_set_hip_error(e_, #x)); } while (0)

struct vbm_decoder {
    vbmd_setup hs;                   // host copy (block sizes, channels); not set in a mixed decoder
    int S = 0, cap = 0, ch = 0;      // ch: channels of a row of every row buffer (mixed: max_channels)
    int halfrate = 0;                // 1: vorbis_synthesis_halfrate
    long half = 0, n1 = 0, ohalf = 0;   // B/2, B >> halfrate, B/2 >> halfrate; B: blocksizes[1] (mixed: max_blocksize)
    int max_classes = 0;             // bytes of partition-class scratch of a row
    int nz = 2;                      // block lists and IMDCT launches per call: one per W (mixed: per block size)
    int size[VBMD_SIZES] = {};       // the block size of list z
    uint8_t *d_setup = nullptr;      // vbmd_setup + blob
    float *d_tables = nullptr;       // fromdB[256], the windows, the trig tables (of size[z] >> halfrate)
    const float *fromdB = nullptr, *win[VBMD_SIZES] = {}, *trig[VBMD_SIZES] = {};
    int *d_ids = nullptr, *d_info = nullptr, *d_fit = nullptr, *d_flags = nullptr, *d_status = nullptr;
    int *d_lists = nullptr, *d_counts = nullptr;
    int *d_runtab = nullptr, *d_plan = nullptr, *d_run_last = nullptr;   // runs: [2S+1], [cap][6], [S]
    int *d_rtab = nullptr, *d_rows = nullptr, *d_zero = nullptr;         // ranges: [4 cap + 1], [cap], [cap] zeros
                                     // (mixed: d_rows [2 cap], the class of every row behind the rows)
    int *d_itab = nullptr;           // device index: [stage_ints] first packets of the streams of one scan launch
    size_t stage_ints = 0;           // ints in a staging slot
    float *d_res = nullptr, *d_spec = nullptr, *d_imdct = nullptr;
    uint8_t *d_cls = nullptr;
    float *d_tail = nullptr;
    int *d_prevW = nullptr;
    long long *d_gp = nullptr, *d_sc = nullptr;
    int *h_stage[kStage] = {};       // max(2S+1, 4 cap + 1) ints each; cap more in a mixed decoder (the rows' classes)
    hipEvent_t ev_stage[kStage] = {};
    int stage_turn = 0;
    std::vector<uint8_t> seen;
    std::vector<int> run_start;
    int last_nsb = 0;
    // mixed decoders (vbm_decoder_create_mixed): the class table, and which class every stream is bound to.  d_ids and
    // d_runtab have cap more ints, the class of every row behind the ids or the run table of the same staging turn.
    struct klass {
        int ch, bs[2];
        std::vector<uint8_t> image;  // vbmd_setup + blob as they lie on the device: the source of the enqueued copy
        uint8_t *d_image;
    };
    int mixed = 0, table_cap = 0;
    std::vector<klass> classes;      // never shrinks, and never grows past table_cap (reserved: entries do not move)
    std::vector<vbmd_class> table;   // host copy of d_table (reserved likewise)
    std::vector<int> scls;           // [S] host mirror of d_scls, -1: not bound
    vbmd_class *d_table = nullptr;
    int *d_scls = nullptr;

    // rcls: in a mixed decoder the device array of the rows' classes; nblocks: rows x channels of the call
    vbmd_launch launch(int nsb, const int *rcls = nullptr, long nblocks = 0) const
    {
        vbmd_launch L;
        L.s = (const vbmd_setup *)d_setup;
        L.blob = d_setup ? d_setup + sizeof(vbmd_setup) : nullptr;
        L.mx = mixed != 0;
        L.M = vbmd_mixed();
        if (mixed) {
            L.M.table = d_table;
            L.M.rcls = rcls;
            L.M.scls = d_scls;
            L.M.CH = ch;
            L.M.cls_bytes = max_classes;
            L.M.list_stride = (long)cap * ch;
            for (int z = 0; z < nz; z++) L.M.win[z] = win[z];
        }
        L.nblocks = mixed ? nblocks : (long)nsb * ch;
        L.nsb = nsb;
        L.ch = ch;
        L.hs = halfrate;
        L.half = half;
        L.n1 = n1;
        L.ohalf = ohalf;
        L.info = d_info;
        L.fit = d_fit;
        L.flags = d_flags;
        L.status = d_status;
        L.lists = d_lists;
        L.counts = d_counts;
        L.res = d_res;
        L.spec = d_spec;
        L.imdct = d_imdct;
        L.cls = d_cls;
        L.fromdB = fromdB;
        L.win0 = win[0];
        L.win1 = win[1];
        L.tail = d_tail;
        L.prevW = d_prevW;
        L.gp = d_gp;
        L.sc = d_sc;
        return L;
    }
};

namespace {

void free_decoder(vbm_decoder *d)
{
    if (!d) return;
    void *bufs[] = {d->d_setup, d->d_tables, d->d_ids, d->d_info, d->d_fit, d->d_flags, d->d_status, d->d_lists,
                    d->d_counts, d->d_res, d->d_spec, d->d_imdct, d->d_cls, d->d_tail, d->d_prevW, d->d_gp, d->d_sc,
                    d->d_runtab, d->d_plan, d->d_run_last, d->d_rtab, d->d_rows, d->d_zero, d->d_itab, d->d_table,
                    d->d_scls};
    for (void *p : bufs)
        if (p) (void)hipFree(p);
    for (const vbm_decoder::klass &k : d->classes)
        if (k.d_image) (void)hipFree(k.d_image);
    for (int i = 0; i < kStage; i++) {
        if (d->h_stage[i]) (void)hipHostFree(d->h_stage[i]);
        if (d->ev_stage[i]) (void)hipEventDestroy(d->ev_stage[i]);
    }
    delete d;
}

// One turn of the staging ring: fill(slot) writes n host ints into the next pinned slot, and they go up to dst
template <class Fill>
int stage(vbm_decoder *d, int *dst, size_t n, hipStream_t q, Fill fill)
{
    const int t = d->stage_turn;
    d->stage_turn = (t + 1) % kStage;
    hipError_t e = hipEventSynchronize(d->ev_stage[t]);      // the copy from kStage turns ago has been done
    if (e != hipSuccess) return vbm_set_hip_error(e, "hipEventSynchronize(stage)");
    fill(d->h_stage[t]);
    e = hipMemcpyAsync(dst, d->h_stage[t], n * sizeof(int), hipMemcpyHostToDevice, q);
    if (e != hipSuccess) return vbm_set_hip_error(e, "hipMemcpyAsync(ids)");
    e = hipEventRecord(d->ev_stage[t], q);
    if (e != hipSuccess) return vbm_set_hip_error(e, "hipEventRecord(stage)");
    return VBM_OK;
}

// n host ints -> dst (d_ids or d_rtab)
int stage_ints(vbm_decoder *d, int *dst, const int *src, size_t n, hipStream_t q)
{
    return stage(d, dst, n, q, [=](int *slot) { memcpy(slot, src, n * sizeof(int)); });
}

int check_ids(vbm_decoder *d, int n, const int *ids)
{
    d->seen.assign(d->S, 0);
    for (int i = 0; i < n; i++) {
        if (ids[i] < 0 || ids[i] >= d->S) { g_vbm_err = "stream id out of range"; return VBM_EINVAL; }
        if (d->seen[ids[i]]) { g_vbm_err = "stream id appears twice in one call"; return VBM_EINVAL; }
        d->seen[ids[i]] = 1;
    }
    return VBM_OK;
}

// the streams of a decode call (check_ids), each of them bound to a class if the decoder is a mixed one
int check_call_ids(vbm_decoder *d, int n, const int *ids)
{
    const int rc = check_ids(d, n, ids);
    if (rc || !d->mixed) return rc;
    for (int i = 0; i < n; i++)
        if (d->scls[ids[i]] < 0) {
            g_vbm_err = "stream " + std::to_string(ids[i]) + " is not bound to a class (vbm_decoder_bind_streams)";
            return VBM_EINVAL;
        }
    return VBM_OK;
}

// an entry point that is not built for mixed decoders, or that has a _mixed form which takes the streams' classes
int refuse_mixed(const vbm_decoder *d, const char *what, const char *instead = nullptr)
{
    if (!d || !d->mixed) return VBM_OK;
    g_vbm_err = instead ? std::string(what) + " of a mixed decoder needs a class per stream: " + instead
                        : std::string(what) + " is not built for a mixed decoder";
    return VBM_EINVAL;
}

// The front of every decode call, over the L.nsb rows of L = d->launch(nsb): the two clears, unpack() (the entry
// point's unpack launch), spectrum and one IMDCT launch per block list.  what: the error text of a failed clear.
template <class Unpack>
int enqueue_front(const vbm_decoder *d, const vbmd_launch &L, hipStream_t q, const char *what, Unpack unpack)
{
    hipError_t e = hipMemsetAsync(d->d_counts, 0, d->nz * sizeof(int), q);
    if (e == hipSuccess) e = hipMemsetAsync(d->d_res, 0, (size_t)L.nsb * d->ch * d->half * sizeof(float), q);
    if (e != hipSuccess) return vbm_set_hip_error(e, what);
    if (unpack()) return VBM_EHIP;
    if (vbmd_launch_spectrum(L, d->d_spec, nullptr, q)) return VBM_EHIP;
    for (int z = 0; z < d->nz; z++)
        if (vbmd_launch_imdct(L, z, d->size[z] >> d->halfrate, d->trig[z], q)) return VBM_EHIP;
    return VBM_OK;
}

// A decoder of one setup (ds), or a mixed one (ds null) with a table of table_cap classes of up to max_channels
// channels and blocks of up to max_blocksize
int create(vbm_decoder **out, const vbm_decode_setup *ds, int table_cap, int max_channels, int max_blocksize,
           int nstreams, int max_batch, int halfrate)
{
    if (!out || nstreams <= 0 || max_batch <= 0) return VBM_EINVAL;
    if (halfrate != 0 && halfrate != 1) { g_vbm_err = "halfrate must be 0 or 1"; return VBM_EINVAL; }
    *out = nullptr;
    const int ndev = vbm_device_count();
    if (ndev < 0) return ndev;
    if (ndev == 0) {
        g_vbm_err = "no HIP device: the MI355X decode path has no CPU fallback";
        return VBM_ENODEV;
    }
    vbm_decoder *d = new vbm_decoder();
    auto fail = [d](int rc) { free_decoder(d); return rc; };
    d->S = nstreams;
    d->cap = max_batch;
    d->halfrate = halfrate;
    d->mixed = ds ? 0 : 1;
    if (ds) {
        d->hs = ds->s;
        d->size[0] = ds->s.blocksizes[0];
        d->size[1] = ds->s.blocksizes[1];
        d->max_classes = ds->s.max_classes;
    } else {
        d->hs = vbmd_setup();
        d->nz = 0;
        for (int bs = 256; bs <= max_blocksize; bs *= 2) d->size[d->nz++] = bs;
        // vbmd_setup_parse's bound for the largest setup the caps allow: one class byte per partition, grouping >= 1
        d->max_classes = max_channels * (max_blocksize / 2);
        d->table_cap = table_cap;
        d->classes.reserve((size_t)table_cap);
        d->table.reserve((size_t)table_cap);
        d->scls.assign((size_t)nstreams, -1);
    }
    d->ch = ds ? ds->s.channels : max_channels;
    const int largest = d->size[d->nz - 1];
    d->half = largest / 2;
    d->n1 = largest >> halfrate;
    d->ohalf = d->half >> halfrate;
    const size_t cap = (size_t)max_batch, ch = (size_t)d->ch;
    if (ds) {
        const size_t setup_bytes = sizeof(vbmd_setup) + ds->blob.size();
        CK(hipMalloc((void **)&d->d_setup, setup_bytes));
        CK(hipMemcpy(d->d_setup, &ds->s, sizeof(vbmd_setup), hipMemcpyHostToDevice));
        if (!ds->blob.empty())
            CK(hipMemcpy(d->d_setup + sizeof(vbmd_setup), ds->blob.data(), ds->blob.size(), hipMemcpyHostToDevice));
    }
    // tables: FLOOR1_fromdB_LOOKUP, the windows, the MDCT trig tables (lib/mdct.c:67-76); at half rate the windows and
    // transforms of half each block size (lib/block.c:208-209, _vorbis_window_get(b->window[W] - hs))
    std::vector<float> tab, mixed_win[VBMD_SIZES];
    if (ds) {
        tab = ds->fromdB;
    } else {
        int sizes[VBMD_SIZES];
        std::vector<float> *wins[VBMD_SIZES];
        for (int z = 0; z < d->nz; z++) {
            sizes[z] = d->size[z] >> halfrate;
            wins[z] = &mixed_win[z];
        }
        const int rc = vbmd_common_tables(&tab, d->nz, sizes, wins);
        if (rc) return fail(rc);
    }
    size_t off_win[VBMD_SIZES], off_trig[VBMD_SIZES];
    for (int z = 0; z < d->nz; z++) {
        const std::vector<float> &win = !ds ? mixed_win[z] : halfrate ? ds->hwin[z] : ds->win[z];
        off_win[z] = tab.size();
        tab.insert(tab.end(), win.begin(), win.end());
    }
    for (int z = 0; z < d->nz; z++) {
        const int n = d->size[z] >> halfrate;
        std::vector<float> t((size_t)n + n / 4);
        vbm_host_mdct_trig(n, t.data());
        while (tab.size() % 4) tab.push_back(0.f);
        off_trig[z] = tab.size();
        tab.insert(tab.end(), t.begin(), t.end());
    }
    CK(hipMalloc((void **)&d->d_tables, tab.size() * sizeof(float)));
    CK(hipMemcpy(d->d_tables, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
    d->fromdB = d->d_tables;
    for (int z = 0; z < d->nz; z++) {
        d->win[z] = d->d_tables + off_win[z];
        d->trig[z] = d->d_tables + off_trig[z];
    }
    const size_t row_classes = d->mixed ? cap : 0;           // the rows' classes travel behind the ids / the run table
    CK(hipMalloc((void **)&d->d_ids, (cap + row_classes) * sizeof(int)));
    CK(hipMalloc((void **)&d->d_info, cap * 4 * sizeof(int)));
    CK(hipMalloc((void **)&d->d_fit, cap * ch * VBMD_POSTS * sizeof(int)));
    CK(hipMalloc((void **)&d->d_flags, cap * ch * sizeof(int)));
    CK(hipMalloc((void **)&d->d_status, cap * sizeof(int)));
    CK(hipMalloc((void **)&d->d_lists, (d->mixed ? d->nz * cap * ch : 2 * cap) * sizeof(int)));
    CK(hipMalloc((void **)&d->d_counts, VBMD_SIZES * sizeof(int)));
    CK(hipMalloc((void **)&d->d_res, cap * ch * d->half * sizeof(float)));
    CK(hipMalloc((void **)&d->d_spec, cap * ch * d->half * sizeof(float)));
    CK(hipMalloc((void **)&d->d_imdct, cap * ch * d->n1 * sizeof(float)));
    CK(hipMalloc((void **)&d->d_cls, cap * (size_t)d->max_classes));
    CK(hipMalloc((void **)&d->d_tail, (size_t)nstreams * ch * d->ohalf * sizeof(float)));
    CK(hipMalloc((void **)&d->d_prevW, (size_t)nstreams * sizeof(int)));
    CK(hipMalloc((void **)&d->d_gp, (size_t)nstreams * sizeof(long long)));
    CK(hipMalloc((void **)&d->d_sc, (size_t)nstreams * sizeof(long long)));
    // range piece tables: at most cap / 2 pieces (each has two rows or more) of 7 ints, and the row starts; in a mixed
    // decoder an eighth int per piece, its class, which 4 cap + 1 holds as well
    const size_t runtab = 2 * (size_t)nstreams + 1 + row_classes, rtab = 4 * cap + 1, stage = rtab > runtab ? rtab : runtab;
    CK(hipMalloc((void **)&d->d_runtab, runtab * sizeof(int)));
    CK(hipMalloc((void **)&d->d_plan, cap * 6 * sizeof(int)));
    CK(hipMalloc((void **)&d->d_run_last, (size_t)nstreams * sizeof(int)));
    CK(hipMalloc((void **)&d->d_rtab, rtab * sizeof(int)));
    CK(hipMalloc((void **)&d->d_rows, (cap + row_classes) * sizeof(int)));
    CK(hipMalloc((void **)&d->d_zero, cap * sizeof(int)));
    CK(hipMemset(d->d_zero, 0, cap * sizeof(int)));
    CK(hipMalloc((void **)&d->d_itab, stage * sizeof(int)));
    d->stage_ints = stage;
    if (d->mixed) {
        CK(hipMalloc((void **)&d->d_table, (size_t)table_cap * sizeof(vbmd_class)));
        CK(hipMemset(d->d_table, 0, (size_t)table_cap * sizeof(vbmd_class)));
        CK(hipMalloc((void **)&d->d_scls, (size_t)nstreams * sizeof(int)));
        CK(hipMemset(d->d_scls, 0xff, (size_t)nstreams * sizeof(int)));
    }
    for (int i = 0; i < kStage; i++) {
        CK(hipHostMalloc((void **)&d->h_stage[i], stage * sizeof(int), hipHostMallocDefault));
        CK(hipEventCreateWithFlags(&d->ev_stage[i], hipEventDisableTiming));
    }
    const int rc = vbm_decoder_reset(d);
    if (rc) return fail(rc);
    *out = d;
    return VBM_OK;
}

}  // namespace

extern "C" int vbm_decoder_create(vbm_decoder **out, const vbm_decode_setup *ds, int nstreams, int max_batch)
{
    return vbm_decoder_create_halfrate(out, ds, nstreams, max_batch, 0);
}

extern "C" int vbm_decoder_halfrate(const vbm_decoder *d) { return d ? d->halfrate : VBM_EINVAL; }

extern "C" int vbm_decoder_create_halfrate(vbm_decoder **out, const vbm_decode_setup *ds, int nstreams, int max_batch,
                                           int halfrate)
{
    if (!ds) return VBM_EINVAL;
    return create(out, ds, 0, 0, 0, nstreams, max_batch, halfrate);
}

extern "C" int vbm_decoder_create_mixed(vbm_decoder **out, int max_classes, int max_channels, int max_blocksize,
                                        int nstreams, int max_batch, int halfrate)
{
    if (max_classes <= 0) { g_vbm_err = "max_classes must be positive"; return VBM_EINVAL; }
    if (max_channels < 1 || max_channels > VBMD_MAXCH) { g_vbm_err = "max_channels must be 1..8"; return VBM_EINVAL; }
    if (max_blocksize < 256 || max_blocksize > 4096 || (max_blocksize & (max_blocksize - 1))) {
        g_vbm_err = "max_blocksize must be a power of two in 256..4096";
        return VBM_EINVAL;
    }
    return create(out, nullptr, max_classes, max_channels, max_blocksize, nstreams, max_batch, halfrate);
}

extern "C" int vbm_decoder_add_class(vbm_decoder *d, const vbm_decode_setup *ds, int *class_id, void *stream)
{
    if (!d || !ds || !class_id) return VBM_EINVAL;
    if (!d->mixed) { g_vbm_err = "vbm_decoder_add_class needs a decoder of vbm_decoder_create_mixed"; return VBM_EINVAL; }
    if (ds->s.channels > d->ch) {
        g_vbm_err = "the class has " + std::to_string(ds->s.channels) + " channels, the decoder's max_channels is " +
                    std::to_string(d->ch);
        return VBM_EINVAL;
    }
    if (ds->s.blocksizes[1] > d->size[d->nz - 1]) {
        g_vbm_err = "the class has blocks of " + std::to_string(ds->s.blocksizes[1]) +
                    ", the decoder's max_blocksize is " + std::to_string(d->size[d->nz - 1]);
        return VBM_EINVAL;
    }
    if (ds->s.max_classes > d->max_classes) { g_vbm_err = "the class needs more partition scratch than the caps give"; return VBM_EINVAL; }
    if ((int)d->classes.size() >= d->table_cap) {
        g_vbm_err = "the class table is full (max_classes " + std::to_string(d->table_cap) + ")";
        return VBM_EINVAL;
    }
    const int id = (int)d->classes.size();
    vbm_decoder::klass k;
    k.ch = ds->s.channels;
    k.bs[0] = ds->s.blocksizes[0];
    k.bs[1] = ds->s.blocksizes[1];
    k.image.resize(sizeof(vbmd_setup) + ds->blob.size());
    memcpy(k.image.data(), &ds->s, sizeof(vbmd_setup));
    if (!ds->blob.empty()) memcpy(k.image.data() + sizeof(vbmd_setup), ds->blob.data(), ds->blob.size());
    k.d_image = nullptr;
    hipError_t e = hipMalloc((void **)&k.d_image, k.image.size());
    if (e != hipSuccess) return vbm_set_hip_error(e, "hipMalloc(class)");
    // slot `id` is new to the device: no call in flight reads it, and no slot below it is written.  The sources of the
    // two copies live as long as the decoder and never move.  They are pageable, so the runtime may stage them before it
    // returns: the copies are ordered on the stream, but the host may wait for the staging.
    d->classes.push_back(std::move(k));
    const vbm_decoder::klass &kk = d->classes.back();
    d->table.push_back({(const vbmd_setup *)kk.d_image, kk.d_image + sizeof(vbmd_setup)});
    hipStream_t q = (hipStream_t)stream;
    e = hipMemcpyAsync(kk.d_image, kk.image.data(), kk.image.size(), hipMemcpyHostToDevice, q);
    if (e == hipSuccess)
        e = hipMemcpyAsync(d->d_table + id, &d->table[id], sizeof(vbmd_class), hipMemcpyHostToDevice, q);
    if (e != hipSuccess) {
        // the host table must not name a class the device slot lacks: wait out whatever copy did start, then take the
        // entry back, so that the next add gets this slot
        (void)hipStreamSynchronize(q);
        (void)hipFree(kk.d_image);
        d->table.pop_back();
        d->classes.pop_back();
        return vbm_set_hip_error(e, "hipMemcpyAsync(class)");
    }
    *class_id = id;
    return VBM_OK;
}

extern "C" int vbm_decoder_bind_streams(vbm_decoder *d, int n, const int *stream_ids, const int *class_ids, void *stream)
{
    if (!d || n < 0 || n > d->cap || (n > 0 && (!stream_ids || !class_ids))) return VBM_EINVAL;
    if (!d->mixed) { g_vbm_err = "vbm_decoder_bind_streams needs a decoder of vbm_decoder_create_mixed"; return VBM_EINVAL; }
    if (n == 0) return VBM_OK;
    int rc = check_ids(d, n, stream_ids);
    if (rc) return rc;
    for (int i = 0; i < n; i++)
        if (class_ids[i] < 0 || class_ids[i] >= (int)d->classes.size()) { g_vbm_err = "class id out of range"; return VBM_EINVAL; }
    hipStream_t q = (hipStream_t)stream;
    rc = stage(d, d->d_ids, 2 * (size_t)n, q, [&](int *slot) {
        memcpy(slot, stream_ids, (size_t)n * sizeof(int));
        memcpy(slot + n, class_ids, (size_t)n * sizeof(int));
    });
    if (rc) return rc;
    if (vbmd_launch_restart(d->d_ids, n, d->d_prevW, d->d_gp, d->d_sc, d->d_ids + n, d->d_scls, q)) return VBM_EHIP;
    for (int i = 0; i < n; i++) d->scls[stream_ids[i]] = class_ids[i];
    return VBM_OK;
}

extern "C" void vbm_decoder_destroy(vbm_decoder *d)
{
    if (!d) return;
    (void)hipDeviceSynchronize();
    free_decoder(d);
}

extern "C" int vbm_decoder_reset(vbm_decoder *d)
{
    if (!d) return VBM_EINVAL;
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemset(d->d_prevW, 0xff, (size_t)d->S * sizeof(int));      // -1: no block yet
    if (e == hipSuccess) e = hipMemset(d->d_gp, 0xff, (size_t)d->S * sizeof(long long));
    if (e == hipSuccess) e = hipMemset(d->d_sc, 0xff, (size_t)d->S * sizeof(long long));
    if (e == hipSuccess) e = hipMemset(d->d_tail, 0, (size_t)d->S * d->ch * d->ohalf * sizeof(float));
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return vbm_set_hip_error(e, "vbm_decoder_reset");
    d->last_nsb = 0;
    return VBM_OK;
}

extern "C" int vbm_decoder_restart_streams(vbm_decoder *d, int n, const int *stream_ids, void *stream)
{
    if (!d || n < 0 || n > d->cap || (n > 0 && !stream_ids)) return VBM_EINVAL;
    if (n == 0) return VBM_OK;
    int rc = check_ids(d, n, stream_ids);
    if (rc) return rc;
    hipStream_t q = (hipStream_t)stream;
    if ((rc = stage_ints(d, d->d_ids, stream_ids, (size_t)n, q))) return rc;
    return vbmd_launch_restart(d->d_ids, n, d->d_prevW, d->d_gp, d->d_sc, nullptr, nullptr, q) ? VBM_EHIP : VBM_OK;
}

extern "C" int vbm_synthesis_batch(vbm_decoder *d, int nsb, const int *stream_ids, const uint8_t *d_packets,
                                   long packet_stride, const int *d_packet_bytes, const long long *d_granulepos,
                                   const uint8_t *d_eos, float *d_pcm, int *d_samples, int *d_status, void *stream)
{
    if (!d || nsb <= 0 || nsb > d->cap || !stream_ids || !d_packets || packet_stride <= 0 || !d_packet_bytes ||
        !d_pcm || !d_samples || !d_status)
        return VBM_EINVAL;
    int rc = check_call_ids(d, nsb, stream_ids);
    if (rc) return rc;
    hipStream_t q = (hipStream_t)stream;
    long nblocks = 0;
    if (d->mixed) {
        rc = stage(d, d->d_ids, 2 * (size_t)nsb, q, [&](int *slot) {                // the ids, then the rows' classes
            memcpy(slot, stream_ids, (size_t)nsb * sizeof(int));
            for (int k = 0; k < nsb; k++) {
                slot[nsb + k] = d->scls[stream_ids[k]];
                nblocks += d->classes[slot[nsb + k]].ch;
            }
        });
    } else {
        rc = stage_ints(d, d->d_ids, stream_ids, (size_t)nsb, q);
    }
    if (rc) return rc;
    const vbmd_launch L = d->launch(nsb, d->d_ids + nsb, nblocks);
    rc = enqueue_front(d, L, q, "hipMemsetAsync(decode)",
                       [&] { return vbmd_launch_unpack(L, d_packets, packet_stride, d_packet_bytes, d_status, q); });
    if (rc) return rc;
    if (vbmd_launch_overlap(L, d->d_ids, d_granulepos, d_eos, d_pcm, d_samples, q)) return VBM_EHIP;
    d->last_nsb = nsb;
    return VBM_OK;
}

extern "C" int vbm_synthesis_runs(vbm_decoder *d, int nruns, const int *stream_ids, const int *run_packets,
                                  const uint8_t *d_data, const long long *d_offsets, long long data_bytes,
                                  const long long *d_granulepos, const uint8_t *d_eos, float *d_pcm, long pcm_stride,
                                  int *d_run_samples, int *d_samples, int *d_status, void *stream)
{
    return vbm_synthesis_runs_gaps(d, nruns, stream_ids, run_packets, d_data, d_offsets, data_bytes, d_granulepos, d_eos,
                                   nullptr, d_pcm, pcm_stride, d_run_samples, d_samples, d_status, stream);
}

extern "C" int vbm_synthesis_runs_gaps(vbm_decoder *d, int nruns, const int *stream_ids, const int *run_packets,
                                       const uint8_t *d_data, const long long *d_offsets, long long data_bytes,
                                       const long long *d_granulepos, const uint8_t *d_eos, const uint8_t *d_gap,
                                       float *d_pcm, long pcm_stride, int *d_run_samples, int *d_samples, int *d_status,
                                       void *stream)
{
    if (!d || nruns < 0 || (nruns > 0 && (!stream_ids || !run_packets)) || data_bytes < 0 ||
        (data_bytes > 0 && !d_data) || !d_offsets || !d_run_samples)
        return VBM_EINVAL;
    if (nruns == 0) return VBM_OK;
    if (nruns > d->S) { g_vbm_err = "more runs than streams"; return VBM_EINVAL; }
    int rc = check_call_ids(d, nruns, stream_ids);
    if (rc) return rc;
    d->run_start.resize((size_t)nruns + 1);
    long long P = 0;
    long need = 0, nblocks = 0;                            // the longest run's samples; rows x channels (mixed)
    for (int r = 0; r < nruns; r++) {
        if (run_packets[r] < 0) { g_vbm_err = "negative packet count"; return VBM_EINVAL; }
        d->run_start[r] = (int)P;
        P += run_packets[r];
        if (P > d->cap) { g_vbm_err = "more packets than max_batch in one call"; return VBM_EINVAL; }
        long row = d->ohalf;
        if (d->mixed) {
            const vbm_decoder::klass &k = d->classes[d->scls[stream_ids[r]]];
            row = k.bs[1] >> (1 + d->halfrate);
            nblocks += (long)run_packets[r] * k.ch;
        }
        need = std::max(need, run_packets[r] * row);
    }
    d->run_start[nruns] = (int)P;
    if (P > 0 && (!d_pcm || !d_samples || !d_status)) return VBM_EINVAL;
    if (pcm_stride < need) {
        g_vbm_err = d->halfrate ? "pcm_stride below max(run_packets) * blocksizes[1]/4"
                                : "pcm_stride below max(run_packets) * blocksizes[1]/2";
        return VBM_EINVAL;
    }
    hipStream_t q = (hipStream_t)stream;
    const int nsb = (int)P;
    const size_t tab = 2 * (size_t)nruns + 1;
    // the run table: ids, then run starts; in a mixed decoder the rows' classes behind it
    rc = stage(d, d->d_runtab, tab + (d->mixed ? (size_t)nsb : 0), q, [&](int *slot) {
        memcpy(slot, stream_ids, (size_t)nruns * sizeof(int));
        memcpy(slot + nruns, d->run_start.data(), ((size_t)nruns + 1) * sizeof(int));
        if (d->mixed)
            for (int r = 0; r < nruns; r++)
                std::fill(slot + tab + d->run_start[r], slot + tab + d->run_start[r + 1], d->scls[stream_ids[r]]);
    });
    if (rc) return rc;
    const vbmd_launch L = d->launch(nsb, d->d_runtab + tab, nblocks);
    rc = enqueue_front(d, L, q, "hipMemsetAsync(decode runs)",
                       [&] { return vbmd_launch_unpack_csr(L, d_data, d_offsets, data_bytes, d_status, q); });
    if (rc) return rc;
    if (vbmd_launch_runs(L, nruns, d->d_runtab, d_granulepos, d_eos, d_gap, d->d_plan, d->d_run_last, d_pcm, pcm_stride,
                         d_run_samples, d_samples, q))
        return VBM_EHIP;
    if (nsb > 0) d->last_nsb = nsb;
    return VBM_OK;
}

extern "C" int vbm_decoder_fetch(vbm_decoder *d, const char *name, void *d_out, long *rows, char *kind, void *stream)
{
    if (refuse_mixed(d, "vbm_decoder_fetch")) return VBM_EINVAL;
    if (!d || !name || d->last_nsb <= 0) return VBM_EINVAL;
    hipStream_t q = (hipStream_t)stream;
    const int nsb = d->last_nsb;
    const size_t plane = (size_t)nsb * d->ch * d->half;
    enum source { COPY, USED, FLOOR };                     // a buffer as it is; from the flags; the floor line from the posts
    const struct { const char *name; long rows; char kind; source from; const void *buf; size_t bytes; } tab[] = {
        {"info", 4, 'i', COPY, d->d_info, (size_t)nsb * 4 * sizeof(int)},
        {"floor_used", 1, 'i', USED, nullptr, 0},
        {"floor_index", d->half, 'i', FLOOR, nullptr, 0},
        {"residue", d->half, 'f', COPY, d->d_res, plane * sizeof(float)},
        {"spectrum", d->half, 'f', COPY, d->d_spec, plane * sizeof(float)}};
    const auto *t = std::find_if(std::begin(tab), std::end(tab), [name](const auto &x) { return !strcmp(name, x.name); });
    if (t == std::end(tab)) { g_vbm_err = std::string("unknown intermediate: ") + name; return VBM_EINVAL; }
    if (rows) *rows = t->rows;
    if (kind) *kind = t->kind;
    if (!d_out) return VBM_OK;
    if (t->from == COPY) {
        const hipError_t e = hipMemcpyAsync(d_out, t->buf, t->bytes, hipMemcpyDeviceToDevice, q);
        return e == hipSuccess ? VBM_OK : vbm_set_hip_error(e, "hipMemcpyAsync(decoder fetch)");
    }
    if (t->from == USED) return vbmd_launch_used(d->d_flags, (int *)d_out, (long)nsb * d->ch, q) ? VBM_EHIP : VBM_OK;
    return vbmd_launch_spectrum(d->launch(nsb), nullptr, (int *)d_out, q) ? VBM_EHIP : VBM_OK;
}

// ---- range stores and range calls ----------------------------------------------------------------------------------
struct vbm_range_store {
    vbm_decoder *dec = nullptr;
    int S = 0;
    std::vector<long long> first;        // [S + 1] first packet of each stream
    std::vector<int> status;             // [P] host index
    std::vector<long long> out_end;      // [P] out_start + samples
    std::vector<long long> totals;       // [S]
    long long data_bytes = 0;
    uint8_t *d_data = nullptr;
    long long *d_offsets = nullptr, *d_out_start = nullptr;   // [P + 1], [P]
    int *d_begin = nullptr, *d_end = nullptr;                 // [P]
    std::vector<int> cls;                // [S] the class of each stream, in a store of a mixed decoder (else empty)
    int halfrate = 0;                    // the decoder's (a host twin's store has no decoder)
    struct vbm_live *live = nullptr;     // a live store's regions, state mirror and workspace (below), else null
};

// A live store (live_store.h) is a vbm_range_store whose streams lie in fixed regions: first[i] = i * (MP + 1), the host
// index (status, out_end) is sized for every slot, and d_data .. d_end are the regions' arrays.  The device form's
// workspace: one pinned table (the entries of an append or restart go up in it; its event says when the copy out of it is
// done), the head's verdicts on the appended packets, the plans, the trimmed list, and the block that comes back in one
// copy: the entries' records, then out_end and status of every new packet (12 B each).
struct vbm_live {
    bool host = false;
    vbml_arrays A = {};                  // device memory, or host memory in the twin
    vbmd_setup hs;                       // twin: the setup
    std::vector<long long> last, lo, bytes;      // [S] mirror: end of the stream's packets, first_sample, retained bytes
    long long trims[2] = {0, 0};         // trims made by the packet cap, by the byte cap
    int *h_tab = nullptr, *d_tab = nullptr, *d_trimmed = nullptr;      // [3 S + 1], [3 S + 1], [S + 1]
    hipEvent_t ev_tab = nullptr;
    vbml_plan *d_plans = nullptr;        // [S]
    size_t pk_cap = 0;                   // packets one append may bring before the next three grow
    int *d_head = nullptr;               // [2 pk_cap] status, W
    uint8_t *d_back = nullptr, *h_back = nullptr;          // [S records + 12 pk_cap]
    std::vector<int> seen;
    std::vector<uint8_t> twin_mem;       // twin: d_head's and d_back's stand-ins
};

namespace {

void free_live(vbm_range_store *st)
{
    vbm_live *lv = st->live;
    void *arrays[] = {lv->A.slots, lv->A.data, lv->A.offsets, lv->A.out_start, lv->A.status, lv->A.begin, lv->A.end};
    for (void *p : arrays)
        if (p) lv->host ? free(p) : (void)hipFree(p);
    void *work[] = {lv->d_tab, lv->d_trimmed, lv->d_plans, lv->d_head, lv->d_back};
    for (void *p : work)
        if (p) (void)hipFree(p);
    if (lv->h_tab) (void)hipHostFree(lv->h_tab);
    if (lv->h_back) (void)hipHostFree(lv->h_back);
    if (lv->ev_tab) (void)hipEventDestroy(lv->ev_tab);
    delete lv;
    st->live = nullptr;
}

void live_view(const vbm_range_store *st, vbm_range_store_view *v)
{
    v->last = st->live->last.data();
    v->lo = st->live->lo.data();
    v->host = st->live->host;
}

}  // namespace

namespace {

void free_store(vbm_range_store *st)
{
    if (!st) return;
    if (st->live) {                      // a live store's arrays are its regions'
        free_live(st);
        delete st;
        return;
    }
    void *bufs[] = {st->d_data, st->d_offsets, st->d_out_start, st->d_begin, st->d_end};
    for (void *p : bufs)
        if (p) (void)hipFree(p);
    delete st;
}

// The argument rules of a range store's CSR, for host arrays (vbm_range_store_create) and device arrays alike
// classes: null (a decoder of one setup), or the class of each stream (a mixed decoder), all of them in its table
int check_csr(const vbm_decoder *d, int nstreams, const long long *stream_packets, const int *classes,
              const uint8_t *data, const long long *offsets, long long data_bytes)
{
    if (!d || nstreams <= 0 || !stream_packets || data_bytes < 0 || (data_bytes > 0 && !data) || !offsets)
        return VBM_EINVAL;
    if (!classes && refuse_mixed(d, "a range store or device index",
                                 "vbm_range_store_create_mixed, _create_device_mixed, vbm_decode_index_device_mixed"))
        return VBM_EINVAL;
    if (classes && !d->mixed) {
        g_vbm_err = "stream classes need a decoder of vbm_decoder_create_mixed";
        return VBM_EINVAL;
    }
    for (int i = 0; classes && i < nstreams; i++)
        if (classes[i] < 0 || classes[i] >= (int)d->classes.size()) {
            g_vbm_err = "stream " + std::to_string(i) + ": class id " + std::to_string(classes[i]) +
                        " is not in the decoder's table (vbm_decoder_add_class)";
            return VBM_EINVAL;
        }
    if (stream_packets[0] != 0) { g_vbm_err = "stream_packets[0] must be 0"; return VBM_EINVAL; }
    for (int i = 0; i < nstreams; i++)
        if (stream_packets[i + 1] < stream_packets[i]) { g_vbm_err = "stream_packets must not decrease"; return VBM_EINVAL; }
    if (stream_packets[nstreams] >= INT_MAX) { g_vbm_err = "more than 2^31 - 2 packets in one store"; return VBM_EINVAL; }
    return VBM_OK;
}

// *out: a store of d for a CSR that check_csr passes, the host index sized, the device arrays allocated, none filled
int new_store(vbm_range_store **out, vbm_decoder *d, int nstreams, const long long *stream_packets, const int *classes,
              const uint8_t *data, const long long *offsets, long long data_bytes)
{
    if (!out) return VBM_EINVAL;
    *out = nullptr;
    const int bad = check_csr(d, nstreams, stream_packets, classes, data, offsets, data_bytes);
    if (bad) return bad;
    const size_t np = (size_t)stream_packets[nstreams];
    vbm_range_store *st = new vbm_range_store();
    auto fail = [st](int rc) { free_store(st); return rc; };
    st->dec = d;
    st->halfrate = d->halfrate;
    st->S = nstreams;
    st->first.assign(stream_packets, stream_packets + nstreams + 1);
    if (classes) st->cls.assign(classes, classes + nstreams);
    st->status.resize(np);
    st->out_end.resize(np);
    st->totals.resize((size_t)nstreams);
    st->data_bytes = data_bytes;
    CK(hipMalloc((void **)&st->d_data, data_bytes > 0 ? (size_t)data_bytes : 1));
    CK(hipMalloc((void **)&st->d_offsets, (np + 1) * sizeof(long long)));
    CK(hipMalloc((void **)&st->d_out_start, (np ? np : 1) * sizeof(long long)));
    CK(hipMalloc((void **)&st->d_begin, (np ? np : 1) * sizeof(int)));
    CK(hipMalloc((void **)&st->d_end, (np ? np : 1) * sizeof(int)));
    *out = st;
    return VBM_OK;
}

// k_index_head over all packets, then k_index_scan over the streams, as many per launch as one staging slot holds
// first packets for (they go up through the ring into d_itab; launches on one stream follow each other).
// classes (a mixed decoder): the streams' classes go up behind their first packets, half as many streams per slot, and
// k_index_head runs behind each upload, over the packets of its streams: one launch over all packets of all classes
// whenever one slot holds the streams, as it does up to 2 * max_batch of them.
int enqueue_index(vbm_decoder *d, int nstreams, const long long *stream_packets, const int *classes,
                  const uint8_t *d_data, const long long *d_offsets, long long data_bytes,
                  const long long *d_granulepos, const uint8_t *d_eos, int *d_status, int *d_begin, int *d_end,
                  long long *d_out_start, long long *d_out_end, long long *d_totals, hipStream_t q)
{
    const vbmd_setup *s = (const vbmd_setup *)d->d_setup;
    if (!classes &&
        vbmd_launch_index_head(s, stream_packets[nstreams], d_data, d_offsets, data_bytes, d_status, d_begin, q))
        return VBM_EHIP;
    const size_t ints = classes ? (d->stage_ints - 1) / 2 : d->stage_ints - 1;
    const int room = (int)std::min<size_t>(ints, (size_t)INT_MAX - 1);
    for (int s0 = 0; s0 < nstreams; s0 += room) {
        const int n = std::min(room, nstreams - s0);
        const int rc = stage(d, d->d_itab, (size_t)n + 1 + (classes ? n : 0), q, [&](int *slot) {
            for (int i = 0; i <= n; i++) slot[i] = (int)stream_packets[s0 + i];
            if (classes) memcpy(slot + n + 1, classes + s0, (size_t)n * sizeof(int));
        });
        if (rc) return rc;
        if (classes && vbmd_launch_index_head_mixed(d->d_table, n, d->d_itab, stream_packets[s0], stream_packets[s0 + n],
                                                    d_data, d_offsets, data_bytes, d_status, d_begin, q))
            return VBM_EHIP;
        if (vbmd_launch_index_scan(s, classes ? d->d_table : nullptr, d->halfrate, n, d->d_itab, d_status, d_granulepos,
                                   d_eos, d_begin, d_end, d_out_start, d_out_end, d_totals + s0, q))
            return VBM_EHIP;
    }
    return VBM_OK;
}

}  // namespace

namespace {

// vbm_range_store_create (classes null) and vbm_range_store_create_mixed
int create_store(vbm_range_store **out, vbm_decoder *d, int nstreams, const long long *stream_packets,
                 const int *classes, const uint8_t *data, const long long *offsets, long long data_bytes,
                 const long long *granulepos, const uint8_t *eos)
{
    const int bad = new_store(out, d, nstreams, stream_packets, classes, data, offsets, data_bytes);
    if (bad) return bad;
    vbm_range_store *st = *out;
    auto fail = [=](int rc) { free_store(st); *out = nullptr; return rc; };
    const size_t np = (size_t)stream_packets[nstreams];
    std::vector<int> begin(np), end(np);
    std::vector<long long> out_start(np);
    for (int i = 0; i < nstreams; i++) {
        const long long a = stream_packets[i];
        // a class's setup is the head of the host image its device copy was made from
        const vbmd_setup &hs = classes ? *(const vbmd_setup *)d->classes[classes[i]].image.data() : d->hs;
        vbmd_index_stream(hs, d->halfrate, stream_packets[i + 1] - a, data, offsets + a, data_bytes,
                          granulepos ? granulepos + a : nullptr, eos ? eos + a : nullptr, st->status.data() + a,
                          begin.data() + a, end.data() + a, out_start.data() + a, &st->totals[i]);
    }
    for (size_t k = 0; k < np; k++) st->out_end[k] = out_start[k] + (end[k] - begin[k]);
    if (data_bytes > 0) CK(hipMemcpy(st->d_data, data, (size_t)data_bytes, hipMemcpyHostToDevice));
    CK(hipMemcpy(st->d_offsets, offsets, (np + 1) * sizeof(long long), hipMemcpyHostToDevice));
    if (np) {
        CK(hipMemcpy(st->d_out_start, out_start.data(), np * sizeof(long long), hipMemcpyHostToDevice));
        CK(hipMemcpy(st->d_begin, begin.data(), np * sizeof(int), hipMemcpyHostToDevice));
        CK(hipMemcpy(st->d_end, end.data(), np * sizeof(int), hipMemcpyHostToDevice));
    }
    return VBM_OK;
}

}  // namespace

extern "C" int vbm_range_store_create(vbm_range_store **out, vbm_decoder *d, int nstreams,
                                      const long long *stream_packets, const uint8_t *data, const long long *offsets,
                                      long long data_bytes, const long long *granulepos, const uint8_t *eos)
{
    return create_store(out, d, nstreams, stream_packets, nullptr, data, offsets, data_bytes, granulepos, eos);
}

extern "C" int vbm_range_store_create_mixed(vbm_range_store **out, vbm_decoder *d, int nstreams,
                                            const long long *stream_packets, const int *stream_classes,
                                            const uint8_t *data, const long long *offsets, long long data_bytes,
                                            const long long *granulepos, const uint8_t *eos)
{
    return create_store(out, d, nstreams, stream_packets, stream_classes, data, offsets, data_bytes, granulepos, eos);
}

extern "C" void vbm_range_store_destroy(vbm_range_store *st)
{
    if (!st) return;
    if (!st->live || !st->live->host) (void)hipDeviceSynchronize();
    free_store(st);
}

void vbm_range_store_get_view(const vbm_range_store *st, vbm_range_store_view *v)
{
    *v = {st->S, st->halfrate, (long long)st->status.size(), st->data_bytes, st->first.data(), st->out_end.data(),
          st->totals.data(), st->first.data() + 1, nullptr, 0, st->status.data(), st->d_data, st->d_offsets,
          st->d_out_start, st->d_begin, st->d_end};
    if (st->live) live_view(st, v);
}

extern "C" int vbm_range_store_totals(const vbm_range_store *st, long long *totals)
{
    if (!st || !totals) return VBM_EINVAL;
    std::copy(st->totals.begin(), st->totals.end(), totals);
    return VBM_OK;
}

extern "C" int vbm_synthesis_ranges(vbm_decoder *d, const vbm_range_store *st, int nranges, const int *stream_ids,
                                    const long long *starts, const int *lengths, float *d_pcm, long pcm_stride,
                                    int *got, void *stream)
{
    if (!d || !st || nranges < 0 || (nranges > 0 && (!stream_ids || !starts || !lengths || !got)))
        return VBM_EINVAL;
    if (st->dec != d) {
        g_vbm_err = st->live && st->live->host ? "a host store (vbm_host_live_store_create) in a device call" : d->mixed ? "the range store was not made for this mixed decoder (vbm_range_store_create_mixed)"
                             : "the range store belongs to another decoder";
        return VBM_EINVAL;
    }
    if (d->cap < 2) { g_vbm_err = "range calls need max_batch >= 2"; return VBM_EINVAL; }
    long most = 0;
    bool any = false;
    for (int r = 0; r < nranges; r++) {
        if (stream_ids[r] < 0 || stream_ids[r] >= st->S) { g_vbm_err = "stream id out of range"; return VBM_EINVAL; }
        if (starts[r] < 0 || lengths[r] < 0) { g_vbm_err = "negative start or length"; return VBM_EINVAL; }
        if (lengths[r] > most) most = lengths[r];
        any |= lengths[r] > 0 && starts[r] < st->totals[stream_ids[r]];
    }
    if (pcm_stride < most) { g_vbm_err = "pcm_stride below max(lengths)"; return VBM_EINVAL; }
    if (any && !d_pcm) return VBM_EINVAL;
    vbm_range_plan plan;
    vbm_range_store_view v;
    vbm_range_store_get_view(st, &v);
    const char *err = vbm_plan_ranges(v.first, v.last, v.lo, v.status, v.out_end, v.totals, d->cap, nranges, stream_ids,
                                      starts, lengths, got, &plan);
    if (err) { g_vbm_err = err; return VBM_EINVAL; }
    hipStream_t q = (hipStream_t)stream;
    std::vector<int> tab;
    for (size_t c = 0; c + 1 < plan.call_first.size(); c++) {
        const int p0 = plan.call_first[c], np = plan.call_first[c + 1] - p0;
        if (np <= 0) continue;
        tab.assign(1, 0);
        for (int p = p0; p < p0 + np; p++) tab.push_back(tab.back() + plan.pieces[p].count + 1);
        const int nsb = tab.back();
        const int r0 = plan.call_r0[c];
        for (int p = p0; p < p0 + np; p++) {
            const vbm_range_piece &pc = plan.pieces[p];
            const unsigned long long s = (unsigned long long)starts[r0 + pc.r];
            tab.insert(tab.end(), {pc.r, pc.pre, pc.first, (int)(unsigned)(s & 0xffffffffu), (int)(unsigned)(s >> 32),
                                   got[r0 + pc.r]});
        }
        long nblocks = 0;                                   // mixed: the pieces' classes, and rows x channels
        for (int p = p0; d->mixed && p < p0 + np; p++) {
            const vbm_range_piece &pc = plan.pieces[p];
            tab.push_back(st->cls[stream_ids[r0 + pc.r]]);
            nblocks += (long)(pc.count + 1) * d->classes[tab.back()].ch;
        }
        int rc = stage_ints(d, d->d_rtab, tab.data(), tab.size(), q);
        if (rc) return rc;
        int *rcls = d->mixed ? d->d_rows + d->cap : nullptr;
        const vbmd_launch L = d->launch(nsb, rcls, nblocks);
        rc = enqueue_front(d, L, q, "hipMemsetAsync(decode ranges)", [&] {
            return vbmd_launch_unpack_rows(L, np, d->d_rtab, d->d_rows, rcls, st->d_data, st->d_offsets, st->data_bytes,
                                           q);
        });
        if (rc) return rc;
        if (vbmd_launch_ranges(L, np, d->d_rtab, d->d_rows, st->d_begin, st->d_end, st->d_out_start, d->d_zero,
                               d->d_plan, d_pcm + (size_t)r0 * d->ch * pcm_stride, pcm_stride, q))
            return VBM_EHIP;
        d->last_nsb = nsb;
    }
    return VBM_OK;
}

// ---- the index and the range store from a CSR in device memory (decode_index.hip) ------------------------------------
extern "C" int vbm_decode_index_device(vbm_decoder *d, int nstreams, const long long *stream_packets,
                                       const uint8_t *d_data, const long long *d_offsets, long long data_bytes,
                                       const long long *d_granulepos, const uint8_t *d_eos, int *d_status, int *d_begin,
                                       int *d_end, long long *d_out_start, long long *d_totals, void *stream)
{
    return vbm_decode_index_device_mixed(d, nstreams, stream_packets, nullptr, d_data, d_offsets, data_bytes,
                                         d_granulepos, d_eos, d_status, d_begin, d_end, d_out_start, d_totals, stream);
}

// stream_classes null: vbm_decode_index_device's body, which refuses a mixed decoder
extern "C" int vbm_decode_index_device_mixed(vbm_decoder *d, int nstreams, const long long *stream_packets,
                                             const int *stream_classes, const uint8_t *d_data,
                                             const long long *d_offsets, long long data_bytes,
                                             const long long *d_granulepos, const uint8_t *d_eos, int *d_status,
                                             int *d_begin, int *d_end, long long *d_out_start, long long *d_totals,
                                             void *stream)
{
    const int rc = check_csr(d, nstreams, stream_packets, stream_classes, d_data, d_offsets, data_bytes);
    if (rc) return rc;
    if (!d_totals || (stream_packets[nstreams] > 0 && (!d_status || !d_begin || !d_end || !d_out_start)))
        return VBM_EINVAL;
    return enqueue_index(d, nstreams, stream_packets, stream_classes, d_data, d_offsets, data_bytes, d_granulepos, d_eos,
                         d_status, d_begin, d_end, d_out_start, nullptr, d_totals, (hipStream_t)stream);
}

extern "C" int vbm_range_store_create_device(vbm_range_store **out, vbm_decoder *d, int nstreams,
                                             const long long *stream_packets, const uint8_t *d_data,
                                             const long long *d_offsets, long long data_bytes,
                                             const long long *d_granulepos, const uint8_t *d_eos, void *stream)
{
    return vbm_range_store_create_device_mixed(out, d, nstreams, stream_packets, nullptr, d_data, d_offsets, data_bytes,
                                               d_granulepos, d_eos, stream);
}

// stream_classes null: vbm_range_store_create_device's body, which refuses a mixed decoder
extern "C" int vbm_range_store_create_device_mixed(vbm_range_store **out, vbm_decoder *d, int nstreams,
                                                   const long long *stream_packets, const int *stream_classes,
                                                   const uint8_t *d_data, const long long *d_offsets,
                                                   long long data_bytes, const long long *d_granulepos,
                                                   const uint8_t *d_eos, void *stream)
{
    int rc = new_store(out, d, nstreams, stream_packets, stream_classes, d_data, d_offsets, data_bytes);
    if (rc) return rc;
    vbm_range_store *st = *out;
    const size_t np = (size_t)stream_packets[nstreams], ns = (size_t)nstreams;
    // what the host planner reads, in one block so that it comes back in one copy: out_end [P], totals [S], status [P]
    const size_t back_bytes = (np + ns) * sizeof(long long) + np * sizeof(int);
    uint8_t *d_back = nullptr;
    hipStream_t q = (hipStream_t)stream;
    auto fail = [&](int rc) {
        (void)hipStreamSynchronize(q);                     // nothing enqueued may still write into the store
        if (d_back) (void)hipFree(d_back);
        free_store(st);
        *out = nullptr;
        return rc;
    };
    CK(hipMalloc((void **)&d_back, back_bytes));
    if (data_bytes > 0) CK(hipMemcpyAsync(st->d_data, d_data, (size_t)data_bytes, hipMemcpyDeviceToDevice, q));
    CK(hipMemcpyAsync(st->d_offsets, d_offsets, (np + 1) * sizeof(long long), hipMemcpyDeviceToDevice, q));
    long long *d_out_end = (long long *)d_back, *d_totals = d_out_end + np;
    int *d_status = (int *)(d_totals + ns);
    rc = enqueue_index(d, nstreams, stream_packets, stream_classes, st->d_data, st->d_offsets, data_bytes, d_granulepos,
                       d_eos, d_status, st->d_begin, st->d_end, st->d_out_start, d_out_end, d_totals, q);
    if (rc) return fail(rc);
    std::vector<uint8_t> back(back_bytes);
    CK(hipMemcpyAsync(back.data(), d_back, back_bytes, hipMemcpyDeviceToHost, q));
    CK(hipStreamSynchronize(q));                           // the one wait: the caller's arrays are free after it
    if (np) memcpy(st->out_end.data(), back.data(), np * sizeof(long long));
    memcpy(st->totals.data(), back.data() + np * sizeof(long long), ns * sizeof(long long));
    if (np) memcpy(st->status.data(), back.data() + (np + ns) * sizeof(long long), np * sizeof(int));
    (void)hipFree(d_back);
    return VBM_OK;
}

// ---- live range stores (live_store.h, live_store.hip) ------------------------------------------------------------------
namespace {

int live_fail(vbm_range_store *st, int rc)
{
    free_store(st);
    return rc;
}

// n zeroed elements in the store's kind of memory
template <class T> int live_get(vbm_live *lv, T *&p, size_t n)
{
    const size_t bytes = (n ? n : 1) * sizeof(T);
    void *v = nullptr;
    if (lv->host) {
        v = calloc(bytes, 1);
        if (!v) { g_vbm_err = "live store: out of host memory"; return VBM_EFAULT; }
    } else {
        hipError_t e = hipMalloc(&v, bytes);
        if (e == hipSuccess) e = hipMemset(v, 0, bytes);
        if (e != hipSuccess) {
            if (v) (void)hipFree(v);
            return vbm_set_hip_error(e, "live store: hipMalloc");
        }
    }
    p = (T *)v;
    return VBM_OK;
}

// room for an append of P packets: the head's arrays and the block that comes back
int live_room(vbm_live *lv, int S, size_t P)
{
    if (P <= lv->pk_cap && (lv->host ? !lv->twin_mem.empty() : lv->d_back != nullptr)) return VBM_OK;
    const size_t cap = std::max(P, std::max<size_t>(2 * lv->pk_cap, 1024));
    const size_t back_bytes = (size_t)S * sizeof(vbml_back) + cap * 12;
    if (lv->host) {
        lv->twin_mem.assign(back_bytes + cap * 2 * sizeof(int), 0);
        lv->pk_cap = cap;
        return VBM_OK;
    }
    if (lv->d_head) (void)hipFree(lv->d_head);
    if (lv->d_back) (void)hipFree(lv->d_back);
    if (lv->h_back) (void)hipHostFree(lv->h_back);
    lv->d_head = nullptr, lv->d_back = lv->h_back = nullptr, lv->pk_cap = 0;
    hipError_t e = hipMalloc((void **)&lv->d_head, cap * 2 * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void **)&lv->d_back, back_bytes);
    if (e == hipSuccess) e = hipHostMalloc((void **)&lv->h_back, back_bytes, hipHostMallocDefault);
    if (e != hipSuccess) return vbm_set_hip_error(e, "vbm_live_store_append: workspace");
    lv->pk_cap = cap;
    return VBM_OK;
}

// ds: the twin's setup (then d is null); classes: a store of a mixed decoder
int live_create(vbm_range_store **out, vbm_decoder *d, const vbm_decode_setup *ds, int halfrate, bool mixed,
                int nstreams, int max_packets, long long max_bytes)
{
    if (!out) return VBM_EINVAL;
    *out = nullptr;
    if (halfrate != 0 && halfrate != 1) { g_vbm_err = "halfrate must be 0 or 1"; return VBM_EINVAL; }
    if ((!d && !ds) || nstreams <= 0 || max_packets <= 0 || max_bytes <= 0) {
        g_vbm_err = "a live store needs a decoder or setup, nstreams, max_packets and max_bytes above 0";
        return VBM_EINVAL;
    }
    if (d && mixed != (d->mixed != 0)) {
        g_vbm_err = mixed ? "vbm_live_store_create_mixed needs a decoder of vbm_decoder_create_mixed"
                          : "a live store of a mixed decoder is made by vbm_live_store_create_mixed";
        return VBM_EINVAL;
    }
    if (max_bytes > INT_MAX - 64 || (long long)nstreams * ((long long)max_packets + 1) >= INT_MAX) {
        g_vbm_err = "a live store holds at most 2^31 - 65 bytes per stream and 2^31 - 2 packet slots in all";
        return VBM_EINVAL;
    }
    vbm_range_store *st = new vbm_range_store();
    vbm_live *lv = st->live = new vbm_live();
    lv->host = d == nullptr;
    if (ds) lv->hs = ds->s;
    st->dec = d;
    st->halfrate = d ? d->halfrate : halfrate;
    st->S = nstreams;
    const size_t S = (size_t)nstreams, slots = S * ((size_t)max_packets + 1);
    vbml_arrays &A = lv->A;
    A.MP = max_packets;
    A.MB = max_bytes;
    A.stride = (max_bytes + 15) & ~15LL;
    st->first.resize(S + 1);
    for (size_t i = 0; i <= S; i++) st->first[i] = (long long)(i * ((size_t)max_packets + 1));
    st->status.assign(slots, 0);
    st->out_end.assign(slots, 0);
    st->totals.assign(S, 0);
    if (mixed) st->cls.assign(S, -1);
    lv->last.assign(st->first.begin(), st->first.begin() + S);
    lv->lo.assign(S, 0);
    lv->bytes.assign(S, 0);
    lv->seen.assign(S, 0);
    st->data_bytes = (long long)S * A.stride;
    int rc = live_get(lv, A.slots, S);
    if (!rc) rc = live_get(lv, A.data, (size_t)st->data_bytes + 16);
    if (!rc) rc = live_get(lv, A.offsets, slots + 1);
    if (!rc) rc = live_get(lv, A.out_start, slots);
    if (!rc) rc = live_get(lv, A.status, slots);
    if (!rc) rc = live_get(lv, A.begin, slots);
    if (!rc) rc = live_get(lv, A.end, slots);
    if (rc) return live_fail(st, rc);
    st->d_data = A.data, st->d_offsets = A.offsets, st->d_out_start = A.out_start, st->d_begin = A.begin, st->d_end = A.end;
    // every slot fresh (class -1 in a mixed store: vbm_live_store_restart gives it one), every region's first offset
    std::vector<vbml_slot> fresh(S, vbml_fresh(mixed ? -1 : 0));
    std::vector<long long> offs(slots + 1, 0);
    for (size_t i = 0; i < S; i++) offs[i * ((size_t)max_packets + 1)] = (long long)i * A.stride;
    if (lv->host) {
        memcpy(A.slots, fresh.data(), S * sizeof(vbml_slot));
        memcpy(A.offsets, offs.data(), offs.size() * sizeof(long long));
        if ((rc = live_room(lv, nstreams, 0))) return live_fail(st, rc);
        *out = st;
        return VBM_OK;
    }
    auto fail = [st](int rc) { return live_fail(st, rc); };
    CK(hipMemcpy(A.slots, fresh.data(), S * sizeof(vbml_slot), hipMemcpyHostToDevice));
    CK(hipMemcpy(A.offsets, offs.data(), offs.size() * sizeof(long long), hipMemcpyHostToDevice));
    CK(hipHostMalloc((void **)&lv->h_tab, (3 * S + 1) * sizeof(int), hipHostMallocDefault));
    CK(hipEventCreateWithFlags(&lv->ev_tab, hipEventDisableTiming));
    CK(hipMalloc((void **)&lv->d_tab, (3 * S + 1) * sizeof(int)));
    CK(hipMalloc((void **)&lv->d_trimmed, (S + 1) * sizeof(int)));
    CK(hipMalloc((void **)&lv->d_plans, S * sizeof(vbml_plan)));
    if ((rc = live_room(lv, nstreams, 0))) return fail(rc);
    *out = st;
    return VBM_OK;
}

// the store's kind, and every id in range and listed once
int live_check(vbm_range_store *st, bool host, int n, const int *ids, const char *who)
{
    if (!st || !st->live) { g_vbm_err = std::string(who) + ": needs a live store"; return VBM_EINVAL; }
    if (st->live->host != host) {
        g_vbm_err = std::string(who) + (host ? ": a device store in a host call" : ": a host store in a device call");
        return VBM_EINVAL;
    }
    if (n < 0 || n > st->S || (n > 0 && !ids)) { g_vbm_err = std::string(who) + ": bad entry count or null ids"; return VBM_EINVAL; }
    std::vector<int> &seen = st->live->seen;
    std::fill(seen.begin(), seen.end(), 0);
    for (int e = 0; e < n; e++) {
        if (ids[e] < 0 || ids[e] >= st->S) { g_vbm_err = std::string(who) + ": stream id out of range"; return VBM_EINVAL; }
        if (seen[ids[e]]) { g_vbm_err = std::string(who) + ": stream id appears twice in one call"; return VBM_EINVAL; }
        seen[ids[e]] = 1;
    }
    return VBM_OK;
}

// the entries of the pinned table: first packets [n + 1], classes [n] (a mixed store), slots [n]
void live_table(const vbm_range_store *st, int n, const int *ids, const int *counts, int *tab)
{
    int P = 0;
    for (int e = 0; e < n; e++) {
        tab[e] = P;
        P += counts[e];
    }
    tab[n] = P;
    const int ids_at = st->cls.empty() ? n + 1 : 2 * n + 1;
    for (int e = 0; e < n; e++) {
        if (!st->cls.empty()) tab[n + 1 + e] = st->cls[ids[e]];
        tab[ids_at + e] = ids[e];
    }
}

// the host's part of an append: the records that came back -> the mirror, and the caller's per-entry arrays
void live_commit(vbm_range_store *st, int n, const int *ids, const int *tab, const vbml_back *back,
                 const long long *pk_out_end, const int *pk_status, int *status, int *dropped, int *retained)
{
    vbm_live *lv = st->live;
    for (int e = 0; e < n; e++) {
        const vbml_back &b = back[e];
        const int sid = ids[e];
        if (status) status[e] = b.status;
        if (dropped) dropped[e] = b.dropped;
        if (retained) retained[e] = b.retained;
        if (b.status) continue;
        const long long P0 = st->first[sid];
        const long long keep = lv->last[sid] - P0 - b.dropped;
        if (b.dropped && keep > 0) {
            memmove(&st->status[P0], &st->status[P0 + b.dropped], (size_t)keep * sizeof(int));
            memmove(&st->out_end[P0], &st->out_end[P0 + b.dropped], (size_t)keep * sizeof(long long));
        }
        const int np = tab[e + 1] - tab[e];
        if (np > 0) {
            memcpy(&st->status[P0 + keep], pk_status + tab[e], (size_t)np * sizeof(int));
            memcpy(&st->out_end[P0 + keep], pk_out_end + tab[e], (size_t)np * sizeof(long long));
        }
        lv->last[sid] = P0 + b.retained;
        lv->lo[sid] = b.first_sample;
        lv->bytes[sid] = b.bytes;
        st->totals[sid] = b.total;
        lv->trims[0] += b.by & 1;
        lv->trims[1] += (b.by >> 1) & 1;
    }
}

// what both appends check of the host arguments; *P: the packets of the call
int live_append_args(vbm_range_store *st, bool host, int n, const int *ids, const int *counts, const uint8_t *data,
                     const long long *offsets, long long data_bytes, long long *P, const char *who)
{
    int rc = live_check(st, host, n, ids, who);
    if (rc) return rc;
    if (data_bytes < 0 || (data_bytes > 0 && !data) || !offsets || (n > 0 && !counts)) {
        g_vbm_err = std::string(who) + ": null pointer or negative data_bytes";
        return VBM_EINVAL;
    }
    *P = 0;
    for (int e = 0; e < n; e++) {
        if (counts[e] < 0) { g_vbm_err = std::string(who) + ": negative packet count"; return VBM_EINVAL; }
        *P += counts[e];
        if (!st->cls.empty() && st->cls[ids[e]] < 0) {
            g_vbm_err = std::string(who) + ": slot " + std::to_string(ids[e]) + " has no class (vbm_live_store_restart)";
            return VBM_EINVAL;
        }
    }
    if (*P >= INT_MAX) { g_vbm_err = std::string(who) + ": more than 2^31 - 2 packets in one call"; return VBM_EINVAL; }
    return VBM_OK;
}

}  // namespace

extern "C" int vbm_live_store_create(vbm_range_store **st, vbm_decoder *dec, int nstreams, int max_packets,
                                     long long max_bytes)
{
    if (!dec) return VBM_EINVAL;
    return live_create(st, dec, nullptr, 0, false, nstreams, max_packets, max_bytes);
}

extern "C" int vbm_live_store_create_mixed(vbm_range_store **st, vbm_decoder *dec, int nstreams, int max_packets,
                                           long long max_bytes)
{
    if (!dec) return VBM_EINVAL;
    return live_create(st, dec, nullptr, 0, true, nstreams, max_packets, max_bytes);
}

extern "C" int vbm_host_live_store_create(vbm_range_store **st, const vbm_decode_setup *ds, int halfrate, int nstreams,
                                          int max_packets, long long max_bytes)
{
    if (!ds) {
        if (halfrate != 0 && halfrate != 1) g_vbm_err = "halfrate must be 0 or 1";
        return VBM_EINVAL;
    }
    return live_create(st, nullptr, ds, halfrate, false, nstreams, max_packets, max_bytes);
}

extern "C" int vbm_live_store_append(vbm_range_store *st, int n, const int *stream_ids, const int *run_packets,
                                     const uint8_t *d_data, const long long *d_offsets, long long data_bytes,
                                     const long long *d_granulepos, const uint8_t *d_eos, const uint8_t *d_gap,
                                     int *status, int *dropped, int *retained, void *stream)
{
    const char *who = "vbm_live_store_append";
    long long P = 0;
    int rc = live_append_args(st, false, n, stream_ids, run_packets, d_data, d_offsets, data_bytes, &P, who);
    if (rc || n == 0) return rc;
    vbm_live *lv = st->live;
    vbm_decoder *d = st->dec;
    hipStream_t q = (hipStream_t)stream;
    if ((rc = live_room(lv, st->S, (size_t)P))) return rc;
    hipError_t e = hipEventSynchronize(lv->ev_tab);         // the last copy out of the table is done
    if (e != hipSuccess) return vbm_set_hip_error(e, "vbm_live_store_append: hipEventSynchronize");
    live_table(st, n, stream_ids, run_packets, lv->h_tab);
    const bool mixed = !st->cls.empty();
    const int ids_at = mixed ? 2 * n + 1 : n + 1;
    e = hipMemcpyAsync(lv->d_tab, lv->h_tab, (size_t)(ids_at + n) * sizeof(int), hipMemcpyHostToDevice, q);
    if (e == hipSuccess) e = hipEventRecord(lv->ev_tab, q);
    if (e != hipSuccess) return vbm_set_hip_error(e, "vbm_live_store_append: upload");
    int *d_head_status = lv->d_head, *d_head_W = lv->d_head + lv->pk_cap;
    vbml_back *d_back = (vbml_back *)lv->d_back;
    long long *d_pk_out_end = (long long *)(d_back + n);
    int *d_pk_status = (int *)(d_pk_out_end + P);
    const vbmd_setup *s = (const vbmd_setup *)d->d_setup;
    if (mixed ? vbmd_launch_index_head_mixed(d->d_table, n, lv->d_tab, 0, P, d_data, d_offsets, data_bytes, d_head_status,
                                             d_head_W, q)
              : vbmd_launch_index_head(s, P, d_data, d_offsets, data_bytes, d_head_status, d_head_W, q))
        return VBM_EHIP;
    if (vbml_launch_append(lv->A, st->halfrate, s, mixed ? d->d_table : nullptr, n, lv->d_tab, ids_at, d_data, d_offsets,
                           data_bytes, d_head_status, d_head_W, d_granulepos, d_eos, d_gap, lv->d_plans, lv->d_trimmed,
                           d_pk_status, d_pk_out_end, d_back, q))
        return VBM_EHIP;
    const size_t back_bytes = (size_t)n * sizeof(vbml_back) + (size_t)P * 12;
    e = hipMemcpyAsync(lv->h_back, lv->d_back, back_bytes, hipMemcpyDeviceToHost, q);
    if (e == hipSuccess) e = hipStreamSynchronize(q);       // the one wait: the caller's arrays are free after it
    if (e != hipSuccess) return vbm_set_hip_error(e, "vbm_live_store_append: read-back");
    const vbml_back *back = (const vbml_back *)lv->h_back;
    const long long *pk_out_end = (const long long *)(back + n);
    live_commit(st, n, stream_ids, lv->h_tab, back, pk_out_end, (const int *)(pk_out_end + P), status, dropped, retained);
    return VBM_OK;
}

extern "C" int vbm_host_live_store_append(vbm_range_store *st, int n, const int *stream_ids, const int *run_packets,
                                          const uint8_t *data, const long long *offsets, long long data_bytes,
                                          const long long *granulepos, const uint8_t *eos, const uint8_t *gap,
                                          int *status, int *dropped, int *retained)
{
    const char *who = "vbm_host_live_store_append";
    long long P = 0;
    int rc = live_append_args(st, true, n, stream_ids, run_packets, data, offsets, data_bytes, &P, who);
    if (rc) return rc;
    bool csr = offsets[0] >= 0 && offsets[P] <= data_bytes;             // the host can see the offsets: all, at once
    for (long long k = 0; k < P && csr; k++) csr = offsets[k + 1] >= offsets[k];
    if (!csr) { g_vbm_err = std::string(who) + ": the offsets are no CSR inside data"; return VBM_EINVAL; }
    if (n == 0) return VBM_OK;
    vbm_live *lv = st->live;
    if ((rc = live_room(lv, st->S, (size_t)P))) return rc;
    std::vector<int> tab(3 * (size_t)n + 1);
    live_table(st, n, stream_ids, run_packets, tab.data());
    vbml_back *back = (vbml_back *)lv->twin_mem.data();
    long long *pk_out_end = (long long *)(back + n);
    int *pk_status = (int *)(pk_out_end + P);
    int *head_status = (int *)(lv->twin_mem.data() + (size_t)st->S * sizeof(vbml_back) + lv->pk_cap * 12);
    int *head_W = head_status + lv->pk_cap;
    for (long long k = 0; k < P; k++) head_status[k] = vbmi_head(lv->hs, data, offsets, data_bytes, k, head_W[k]);
    for (int e = 0; e < n; e++) {
        const auto entry = st->halfrate ? vbml_host_append_entry<1> : vbml_host_append_entry<0>;
        entry(lv->A, lv->hs.blocksizes, stream_ids[e], tab[e], tab[e + 1], data, offsets, data_bytes, head_status, head_W,
              granulepos, eos, gap, pk_status, pk_out_end, back[e]);
    }
    live_commit(st, n, stream_ids, tab.data(), back, pk_out_end, pk_status, status, dropped, retained);
    return VBM_OK;
}

namespace {

// both restarts: the slots fresh, in a mixed store of the classes given
int live_restart(vbm_range_store *st, bool host, int n, const int *ids, const int *classes, hipStream_t q, const char *who)
{
    int rc = live_check(st, host, n, ids, who);
    if (rc) return rc;
    vbm_live *lv = st->live;
    const bool mixed = !st->cls.empty();
    if (mixed != (classes != nullptr) && n > 0) {
        g_vbm_err = std::string(who) + (mixed ? ": a store of a mixed decoder needs the slots' classes"
                                              : ": classes need a store of a mixed decoder");
        return VBM_EINVAL;
    }
    for (int e = 0; mixed && e < n; e++)
        if (classes[e] < 0 || classes[e] >= (int)st->dec->classes.size()) {
            g_vbm_err = std::string(who) + ": class id " + std::to_string(classes[e]) + " is not in the decoder's table";
            return VBM_EINVAL;
        }
    if (n == 0) return VBM_OK;
    if (host) {
        for (int e = 0; e < n; e++) lv->A.slots[ids[e]] = vbml_fresh(0);
    } else {
        hipError_t e = hipEventSynchronize(lv->ev_tab);
        if (e != hipSuccess) return vbm_set_hip_error(e, "vbm_live_store_restart: hipEventSynchronize");
        memcpy(lv->h_tab, ids, (size_t)n * sizeof(int));
        if (mixed) memcpy(lv->h_tab + n, classes, (size_t)n * sizeof(int));
        e = hipMemcpyAsync(lv->d_tab, lv->h_tab, (size_t)(mixed ? 2 : 1) * n * sizeof(int), hipMemcpyHostToDevice, q);
        if (e == hipSuccess) e = hipEventRecord(lv->ev_tab, q);
        if (e != hipSuccess) return vbm_set_hip_error(e, "vbm_live_store_restart: upload");
        if (vbml_launch_restart(lv->A, n, lv->d_tab, mixed ? lv->d_tab + n : nullptr, q)) return VBM_EHIP;
    }
    for (int e = 0; e < n; e++) {
        const int sid = ids[e];
        lv->last[sid] = st->first[sid];
        lv->lo[sid] = lv->bytes[sid] = st->totals[sid] = 0;
        if (mixed) st->cls[sid] = classes[e];
    }
    return VBM_OK;
}

}  // namespace

extern "C" int vbm_live_store_restart(vbm_range_store *st, int n, const int *stream_ids, const int *classes, void *stream)
{
    return live_restart(st, false, n, stream_ids, classes, (hipStream_t)stream, "vbm_live_store_restart");
}

extern "C" int vbm_host_live_store_restart(vbm_range_store *st, int n, const int *stream_ids)
{
    return live_restart(st, true, n, stream_ids, nullptr, nullptr, "vbm_host_live_store_restart");
}

extern "C" int vbm_live_store_state(const vbm_range_store *st, long long *first_sample, long long *totals,
                                    long long *packets, long long *bytes, long long *trims)
{
    if (!st || !st->live) { g_vbm_err = "vbm_live_store_state: needs a live store"; return VBM_EINVAL; }
    const vbm_live *lv = st->live;
    for (int i = 0; i < st->S; i++) {
        if (first_sample) first_sample[i] = lv->lo[i];
        if (totals) totals[i] = st->totals[i];
        if (packets) packets[i] = lv->last[i] - st->first[i];
        if (bytes) bytes[i] = lv->bytes[i];
    }
    if (trims) trims[0] = lv->trims[0], trims[1] = lv->trims[1];
    return VBM_OK;
}

extern "C" int vbm_host_live_store_state(const vbm_range_store *st, long long *first_sample, long long *totals,
                                         long long *packets, long long *bytes, long long *trims)
{
    return vbm_live_store_state(st, first_sample, totals, packets, bytes, trims);
}

namespace {

// Both snapshots.  The index of the retained packets is the host mirror's; begin, the offsets and the bytes come out of
// the regions, stream after stream (device form: behind a wait for `q`, one blocking copy per array and stream).
int live_snapshot(const vbm_range_store *st, bool host, long long *first, int *status, int *begin, long long *out_end,
                  long long *totals, uint8_t *data, long long *offsets, hipStream_t q, const char *who)
{
    if (!st || !st->live || st->live->host != host) {
        g_vbm_err = std::string(who) + (host ? ": needs a store of vbm_host_live_store_create"
                                             : ": needs a store of vbm_live_store_create");
        return VBM_EINVAL;
    }
    if (!first || !totals || !offsets) return VBM_EINVAL;
    const vbm_live *lv = st->live;
    const vbml_arrays &A = lv->A;
    if (!host) {
        const hipError_t e = hipStreamSynchronize(q);
        if (e != hipSuccess) return vbm_set_hip_error(e, "vbm_live_store_snapshot: hipStreamSynchronize");
    }
    auto fetch = [&](void *dst, const void *src, size_t bytes) {
        if (!bytes) return hipSuccess;
        if (host) { memcpy(dst, src, bytes); return hipSuccess; }
        return hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
    };
    long long at = 0, byte = 0;
    std::vector<long long> off;
    first[0] = 0;
    offsets[0] = 0;
    for (int i = 0; i < st->S; i++) {
        const long long P0 = st->first[i], n = lv->last[i] - P0, nb = lv->bytes[i];
        if (n > 0 && (!status || !begin || !out_end)) return VBM_EINVAL;
        if (nb > 0 && !data) return VBM_EINVAL;
        off.resize((size_t)n + 1);
        hipError_t e = fetch(off.data(), A.offsets + P0, ((size_t)n + 1) * sizeof(long long));
        if (e == hipSuccess) e = fetch(begin + at, A.begin + P0, (size_t)n * sizeof(int));
        if (e == hipSuccess) e = fetch(data + byte, A.data + (long long)i * A.stride, (size_t)nb);
        if (e != hipSuccess) return vbm_set_hip_error(e, "vbm_live_store_snapshot: copy");
        for (long long k = 0; k < n; k++) {
            status[at + k] = st->status[P0 + k];
            out_end[at + k] = st->out_end[P0 + k];
            offsets[at + k + 1] = byte + (off[k + 1] - off[0]);
        }
        totals[i] = st->totals[i];
        at += n;
        byte += nb;
        first[i + 1] = at;
    }
    return VBM_OK;
}

}  // namespace

extern "C" int vbm_live_store_snapshot(const vbm_range_store *st, long long *first, int *status, int *begin,
                                       long long *out_end, long long *totals, uint8_t *data, long long *offsets,
                                       void *stream)
{
    return live_snapshot(st, false, first, status, begin, out_end, totals, data, offsets, (hipStream_t)stream,
                         "vbm_live_store_snapshot");
}

extern "C" int vbm_host_live_store_snapshot(const vbm_range_store *st, long long *first, int *status, int *begin,
                                            long long *out_end, long long *totals, uint8_t *data, long long *offsets)
{
    return live_snapshot(st, true, first, status, begin, out_end, totals, data, offsets, nullptr,
                         "vbm_host_live_store_snapshot");
}
