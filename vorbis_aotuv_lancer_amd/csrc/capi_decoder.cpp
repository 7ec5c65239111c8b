// C ABI of the batched device decoder (include/vorbis_mi355x.h, "decode" section).
//
// One vbm_synthesis_batch call enqueues, on the caller's stream: the upload of the row -> stream map (pinned staging),
// k_unpack (entropy decode, row lists by block size), k_spectrum, one k_imdct launch per block size (each reads its row
// count from the device: rows of mixed block size are never sorted on the host) and k_overlap.  Nothing waits on
// the device, except a staging slot that is still in flight from four calls back.
//
// vbm_synthesis_runs enqueues the same unpack (from CSR offsets), spectrum and IMDCT launches over rows that are runs of
// consecutive packets of one stream, then k_run_plan, k_overlap_runs and k_run_commit in place of k_overlap.  The run
// table (stream ids and run starts) goes up through the same staging ring.
#include <cstring>
#include <string>
#include <vector>

#include "decode_kernels.h"
#include "decode_setup.h"
#include "vbm_internal.h"
#include "vorbis_mi355x.h"

extern "C" int vbm_host_mdct_trig(int n, float *out);

namespace {
constexpr int kStage = 4;
}

struct vbm_decoder {
    vbmd_setup hs;                   // host copy (block sizes, channels)
    int S = 0, cap = 0, ch = 0;
    long half = 0, n1 = 0;
    int max_classes = 0;
    uint8_t *d_setup = nullptr;      // vbmd_setup + blob
    float *d_tables = nullptr;       // fromdB[256], win0, win1, trig0, trig1
    const float *fromdB = nullptr, *win[2] = {}, *trig[2] = {};
    int *d_ids = nullptr, *d_info = nullptr, *d_fit = nullptr, *d_flags = nullptr, *d_status = nullptr;
    int *d_lists = nullptr, *d_counts = nullptr;
    int *d_runtab = nullptr, *d_plan = nullptr, *d_run_last = nullptr;   // runs: [2S+1], [cap][6], [S]
    float *d_res = nullptr, *d_spec = nullptr, *d_imdct = nullptr;
    uint8_t *d_cls = nullptr;
    float *d_tail = nullptr;
    int *d_prevW = nullptr;
    long long *d_gp = nullptr, *d_sc = nullptr;
    int *h_stage[kStage] = {};       // max(cap, 2S+1) ints each
    hipEvent_t ev_stage[kStage] = {};
    int stage_turn = 0;
    std::vector<uint8_t> seen;
    std::vector<int> run_start;
    int last_nsb = 0;

    vbmd_launch launch(int nsb) const
    {
        vbmd_launch L;
        L.s = (const vbmd_setup *)d_setup;
        L.blob = d_setup + sizeof(vbmd_setup);
        L.nsb = nsb;
        L.ch = ch;
        L.half = half;
        L.n1 = n1;
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
                    d->d_runtab, d->d_plan, d->d_run_last};
    for (void *p : bufs)
        if (p) (void)hipFree(p);
    for (int i = 0; i < kStage; i++) {
        if (d->h_stage[i]) (void)hipHostFree(d->h_stage[i]);
        if (d->ev_stage[i]) (void)hipEventDestroy(d->ev_stage[i]);
    }
    delete d;
}

// host ints -> dst (d_ids or d_runtab) through the next pinned staging slot
int stage_ints(vbm_decoder *d, int *dst, const int *const *parts, const int *lens, int nparts, hipStream_t q)
{
    const int t = d->stage_turn;
    d->stage_turn = (t + 1) % kStage;
    hipError_t e = hipEventSynchronize(d->ev_stage[t]);      // the copy from kStage calls ago has been done
    if (e != hipSuccess) return vbm_set_hip_error(e, "hipEventSynchronize(stage)");
    size_t n = 0;
    for (int i = 0; i < nparts; i++) {
        memcpy(d->h_stage[t] + n, parts[i], (size_t)lens[i] * sizeof(int));
        n += (size_t)lens[i];
    }
    e = hipMemcpyAsync(dst, d->h_stage[t], n * sizeof(int), hipMemcpyHostToDevice, q);
    if (e != hipSuccess) return vbm_set_hip_error(e, "hipMemcpyAsync(ids)");
    e = hipEventRecord(d->ev_stage[t], q);
    if (e != hipSuccess) return vbm_set_hip_error(e, "hipEventRecord(stage)");
    return VBM_OK;
}

int stage_ids(vbm_decoder *d, const int *ids, int n, hipStream_t q) { return stage_ints(d, d->d_ids, &ids, &n, 1, q); }

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

}  // namespace

extern "C" int vbm_decoder_create(vbm_decoder **out, const vbm_decode_setup *ds, int nstreams, int max_batch)
{
    if (!out || !ds || nstreams <= 0 || max_batch <= 0) return VBM_EINVAL;
    *out = nullptr;
    const int ndev = vbm_device_count();
    if (ndev < 0) return ndev;
    if (ndev == 0) {
        g_vbm_err = "no HIP device: the MI355X decode path has no CPU fallback";
        return VBM_ENODEV;
    }
    vbm_decoder *d = new vbm_decoder();
    d->hs = ds->s;
    d->S = nstreams;
    d->cap = max_batch;
    d->ch = ds->s.channels;
    d->n1 = ds->s.blocksizes[1];
    d->half = d->n1 / 2;
    d->max_classes = ds->s.max_classes;
    const size_t cap = (size_t)max_batch, ch = (size_t)d->ch;
    hipError_t e = hipSuccess;
#define CK(x) do { e = (x); if (e != hipSuccess) { int rc = vbm_set_hip_error(e, #x); free_decoder(d); return rc; } } while (0)
    const size_t setup_bytes = sizeof(vbmd_setup) + ds->blob.size();
    CK(hipMalloc((void **)&d->d_setup, setup_bytes));
    CK(hipMemcpy(d->d_setup, &ds->s, sizeof(vbmd_setup), hipMemcpyHostToDevice));
    if (!ds->blob.empty())
        CK(hipMemcpy(d->d_setup + sizeof(vbmd_setup), ds->blob.data(), ds->blob.size(), hipMemcpyHostToDevice));
    // tables: FLOOR1_fromdB_LOOKUP, the two windows, the two MDCT trig tables (lib/mdct.c:67-76)
    std::vector<float> tab(ds->fromdB);
    size_t off_win[2], off_trig[2];
    for (int w = 0; w < 2; w++) { off_win[w] = tab.size(); tab.insert(tab.end(), ds->win[w].begin(), ds->win[w].end()); }
    for (int w = 0; w < 2; w++) {
        const int n = ds->s.blocksizes[w];
        std::vector<float> t((size_t)n + n / 4);
        vbm_host_mdct_trig(n, t.data());
        while (tab.size() % 4) tab.push_back(0.f);
        off_trig[w] = tab.size();
        tab.insert(tab.end(), t.begin(), t.end());
    }
    CK(hipMalloc((void **)&d->d_tables, tab.size() * sizeof(float)));
    CK(hipMemcpy(d->d_tables, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
    d->fromdB = d->d_tables;
    for (int w = 0; w < 2; w++) {
        d->win[w] = d->d_tables + off_win[w];
        d->trig[w] = d->d_tables + off_trig[w];
    }
    CK(hipMalloc((void **)&d->d_ids, cap * sizeof(int)));
    CK(hipMalloc((void **)&d->d_info, cap * 4 * sizeof(int)));
    CK(hipMalloc((void **)&d->d_fit, cap * ch * VBMD_POSTS * sizeof(int)));
    CK(hipMalloc((void **)&d->d_flags, cap * ch * sizeof(int)));
    CK(hipMalloc((void **)&d->d_status, cap * sizeof(int)));
    CK(hipMalloc((void **)&d->d_lists, 2 * cap * sizeof(int)));
    CK(hipMalloc((void **)&d->d_counts, 2 * sizeof(int)));
    CK(hipMalloc((void **)&d->d_res, cap * ch * d->half * sizeof(float)));
    CK(hipMalloc((void **)&d->d_spec, cap * ch * d->half * sizeof(float)));
    CK(hipMalloc((void **)&d->d_imdct, cap * ch * d->n1 * sizeof(float)));
    CK(hipMalloc((void **)&d->d_cls, cap * (size_t)d->max_classes));
    CK(hipMalloc((void **)&d->d_tail, (size_t)nstreams * ch * d->half * sizeof(float)));
    CK(hipMalloc((void **)&d->d_prevW, (size_t)nstreams * sizeof(int)));
    CK(hipMalloc((void **)&d->d_gp, (size_t)nstreams * sizeof(long long)));
    CK(hipMalloc((void **)&d->d_sc, (size_t)nstreams * sizeof(long long)));
    const size_t runtab = 2 * (size_t)nstreams + 1, stage = cap > runtab ? cap : runtab;
    CK(hipMalloc((void **)&d->d_runtab, runtab * sizeof(int)));
    CK(hipMalloc((void **)&d->d_plan, cap * 6 * sizeof(int)));
    CK(hipMalloc((void **)&d->d_run_last, (size_t)nstreams * sizeof(int)));
    for (int i = 0; i < kStage; i++) {
        CK(hipHostMalloc((void **)&d->h_stage[i], stage * sizeof(int), hipHostMallocDefault));
        CK(hipEventCreateWithFlags(&d->ev_stage[i], hipEventDisableTiming));
    }
#undef CK
    const int rc = vbm_decoder_reset(d);
    if (rc) { free_decoder(d); return rc; }
    *out = d;
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
    if (e == hipSuccess) e = hipMemset(d->d_tail, 0, (size_t)d->S * d->ch * d->half * sizeof(float));
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
    if ((rc = stage_ids(d, stream_ids, n, q))) return rc;
    return vbmd_launch_restart(d->d_ids, n, d->d_prevW, d->d_gp, d->d_sc, q) ? VBM_EHIP : VBM_OK;
}

extern "C" int vbm_synthesis_batch(vbm_decoder *d, int nsb, const int *stream_ids, const uint8_t *d_packets,
                                   long packet_stride, const int *d_packet_bytes, const long long *d_granulepos,
                                   const uint8_t *d_eos, float *d_pcm, int *d_samples, int *d_status, void *stream)
{
    if (!d || nsb <= 0 || nsb > d->cap || !stream_ids || !d_packets || packet_stride <= 0 || !d_packet_bytes ||
        !d_pcm || !d_samples || !d_status)
        return VBM_EINVAL;
    int rc = check_ids(d, nsb, stream_ids);
    if (rc) return rc;
    hipStream_t q = (hipStream_t)stream;
    if ((rc = stage_ids(d, stream_ids, nsb, q))) return rc;
    hipError_t e = hipMemsetAsync(d->d_counts, 0, 2 * sizeof(int), q);
    if (e == hipSuccess) e = hipMemsetAsync(d->d_res, 0, (size_t)nsb * d->ch * d->half * sizeof(float), q);
    if (e != hipSuccess) return vbm_set_hip_error(e, "hipMemsetAsync(decode)");
    const vbmd_launch L = d->launch(nsb);
    if (vbmd_launch_unpack(L, d_packets, packet_stride, d_packet_bytes, d_status, q)) return VBM_EHIP;
    if (vbmd_launch_spectrum(L, d->d_spec, nullptr, q)) return VBM_EHIP;
    for (int W = 0; W < 2; W++)
        if (vbmd_launch_imdct(L, W, d->hs.blocksizes[W], d->trig[W], q)) return VBM_EHIP;
    if (vbmd_launch_overlap(L, d->d_ids, d_granulepos, d_eos, d_pcm, d_samples, q)) return VBM_EHIP;
    d->last_nsb = nsb;
    return VBM_OK;
}

extern "C" int vbm_synthesis_runs(vbm_decoder *d, int nruns, const int *stream_ids, const int *run_packets,
                                  const uint8_t *d_data, const long long *d_offsets, long long data_bytes,
                                  const long long *d_granulepos, const uint8_t *d_eos, float *d_pcm, long pcm_stride,
                                  int *d_run_samples, int *d_samples, int *d_status, void *stream)
{
    if (!d || nruns < 0 || (nruns > 0 && (!stream_ids || !run_packets)) || data_bytes < 0 ||
        (data_bytes > 0 && !d_data) || !d_offsets || !d_run_samples)
        return VBM_EINVAL;
    if (nruns == 0) return VBM_OK;
    if (nruns > d->S) { g_vbm_err = "more runs than streams"; return VBM_EINVAL; }
    int rc = check_ids(d, nruns, stream_ids);
    if (rc) return rc;
    d->run_start.resize((size_t)nruns + 1);
    long long P = 0;
    int most = 0;
    for (int r = 0; r < nruns; r++) {
        if (run_packets[r] < 0) { g_vbm_err = "negative packet count"; return VBM_EINVAL; }
        d->run_start[r] = (int)P;
        P += run_packets[r];
        if (P > d->cap) { g_vbm_err = "more packets than max_batch in one call"; return VBM_EINVAL; }
        if (run_packets[r] > most) most = run_packets[r];
    }
    d->run_start[nruns] = (int)P;
    if (P > 0 && (!d_pcm || !d_samples || !d_status)) return VBM_EINVAL;
    if (pcm_stride < (long)most * d->half) { g_vbm_err = "pcm_stride below max(run_packets) * blocksizes[1]/2"; return VBM_EINVAL; }
    hipStream_t q = (hipStream_t)stream;
    const int *parts[2] = {stream_ids, d->run_start.data()};
    const int lens[2] = {nruns, nruns + 1};
    if ((rc = stage_ints(d, d->d_runtab, parts, lens, 2, q))) return rc;
    const int nsb = (int)P;
    hipError_t e = hipMemsetAsync(d->d_counts, 0, 2 * sizeof(int), q);
    if (e == hipSuccess) e = hipMemsetAsync(d->d_res, 0, (size_t)nsb * d->ch * d->half * sizeof(float), q);
    if (e != hipSuccess) return vbm_set_hip_error(e, "hipMemsetAsync(decode runs)");
    const vbmd_launch L = d->launch(nsb);
    if (vbmd_launch_unpack_csr(L, d_data, d_offsets, data_bytes, d_status, q)) return VBM_EHIP;
    if (vbmd_launch_spectrum(L, d->d_spec, nullptr, q)) return VBM_EHIP;
    for (int W = 0; W < 2; W++)
        if (vbmd_launch_imdct(L, W, d->hs.blocksizes[W], d->trig[W], q)) return VBM_EHIP;
    if (vbmd_launch_runs(L, nruns, d->d_runtab, d_granulepos, d_eos, d->d_plan, d->d_run_last, d_pcm, pcm_stride,
                         d_run_samples, d_samples, q))
        return VBM_EHIP;
    if (nsb > 0) d->last_nsb = nsb;
    return VBM_OK;
}

extern "C" int vbm_decoder_fetch(vbm_decoder *d, const char *name, void *d_out, long *rows, char *kind, void *stream)
{
    if (!d || !name || d->last_nsb <= 0) return VBM_EINVAL;
    hipStream_t q = (hipStream_t)stream;
    const int nsb = d->last_nsb;
    const size_t plane = (size_t)nsb * d->ch * d->half;
    const vbmd_launch L = d->launch(nsb);
    long r;
    char k;
    if (!strcmp(name, "info")) { r = 4; k = 'i'; }
    else if (!strcmp(name, "floor_used")) { r = 1; k = 'i'; }
    else if (!strcmp(name, "floor_index")) { r = d->half; k = 'i'; }
    else if (!strcmp(name, "residue") || !strcmp(name, "spectrum")) { r = d->half; k = 'f'; }
    else { g_vbm_err = std::string("unknown intermediate: ") + name; return VBM_EINVAL; }
    if (rows) *rows = r;
    if (kind) *kind = k;
    if (!d_out) return VBM_OK;
    hipError_t e = hipSuccess;
    if (!strcmp(name, "info")) e = hipMemcpyAsync(d_out, d->d_info, (size_t)nsb * 4 * sizeof(int), hipMemcpyDeviceToDevice, q);
    else if (!strcmp(name, "residue")) e = hipMemcpyAsync(d_out, d->d_res, plane * sizeof(float), hipMemcpyDeviceToDevice, q);
    else if (!strcmp(name, "spectrum")) e = hipMemcpyAsync(d_out, d->d_spec, plane * sizeof(float), hipMemcpyDeviceToDevice, q);
    else if (!strcmp(name, "floor_used")) return vbmd_launch_used(d->d_flags, (int *)d_out, (long)nsb * d->ch, q) ? VBM_EHIP : VBM_OK;
    else return vbmd_launch_spectrum(L, nullptr, (int *)d_out, q) ? VBM_EHIP : VBM_OK;   // floor line from the posts
    return e == hipSuccess ? VBM_OK : vbm_set_hip_error(e, "hipMemcpyAsync(decoder fetch)");
}
