// The Vorbis stream of multiplexed Ogg files, picked on the device for many files per call (rule and workspace:
// ogg_select.h), the host twin, and the C ABI over both (include/vorbis_mi355x.h, "Ogg stream selection"; host scaffold:
// twin_host.h).
//
//   k_sel_walk   one wavefront per file, page after page, as k_chain_walk: every lane loads one header byte and four
//                bytes behind the header in one round trip.  Those 256 bytes hold the lacing values and, for a page of
//                up to 244 segments, the first bytes of the body as well, so a head page shows its mark without a second
//                round trip (a Vorbis identification page has one segment); a head page with more segments takes one
//                more.  The state is uniform over the wavefront; lane 0 writes the run records and the file's counts
//   k_sel_scan   one block, four files per thread: exclusive scan of the kept bytes -> d_out_offsets; the capacity check
//   k_sel_copy   block b writes bytes [b * CHUNK, (b + 1) * CHUNK) of the whole output: it finds the file of its first
//                byte by a search in d_out_offsets and the run by a search in that file's records, then goes from run to
//                run.  16-byte stores aligned on the destination; the source is read as aligned 16-byte words and
//                shifted by its byte offset; the few bytes at the ends of a run's part go one by one.  No LDS.
//                The run counts need no scan: a file's records lie at its own slot (ogg_select.h), and nothing asks for
//                their total
#include <hip/hip_runtime.h>
#include <string.h>
#include <new>
#include <string>

#include "ogg_emit.h"
#include "ogg_select.h"
#include "twin_host.h"

namespace {

constexpr int kChunk = VBM_OGG_SELECT_CHUNK;

// ---- kernels ---------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(64) k_sel_walk(const uint8_t *data, const long long *off, OggSelRun *runs, long long *nruns,
                                                 long long *kept, vbm_ogg_select_info *info)
{
    const int f = blockIdx.x, lane = threadIdx.x;
    const long long begin = off[f], end = off[f + 1];
    const long long slot = oggdmx_first_slot(off, f), room = oggdmx_first_slot(off, f + 1) - slot;
    OggSelWalk w;                                   // the same in every lane, as is every exit below
    oggsel_begin(w);
    long long pos = begin;
    bool room_left = true;
    while (room_left) {
        const long long left = end - pos;
        if (left < 27) break;
        const uint8_t *h = data + pos;
        // the round trip: header byte `lane`, and bytes 27 + 4 * lane .. 27 + 4 * lane + 3 of the page if the file goes on
        // that far: lacing values, and behind them the body
        const int hb = lane < 27 ? h[lane] : 0;
        const uint32_t lw = dmx_load4(h + 27 + 4 * lane, left - 27 - 4 * lane);
        const uint32_t capture = (uint32_t)__builtin_amdgcn_readlane(hb, 0) | ((uint32_t)__builtin_amdgcn_readlane(hb, 1) << 8) |
                                 ((uint32_t)__builtin_amdgcn_readlane(hb, 2) << 16) |
                                 ((uint32_t)__builtin_amdgcn_readlane(hb, 3) << 24);
        if (!oggchain_header_ok(capture, __builtin_amdgcn_readlane(hb, 4))) break;
        const int flags = __builtin_amdgcn_readlane(hb, 5), nseg = __builtin_amdgcn_readlane(hb, 26);
        if (!oggchain_lacing_fits(left, nseg)) break;
        const int mine = min(4, max(0, nseg - 4 * lane));           // how many of my four are lacing values
        const uint32_t v = mine == 4 ? lw : lw & ((1u << (8 * mine)) - 1u);
        int body = (int)((v & 0xff) + ((v >> 8) & 0xff) + ((v >> 16) & 0xff) + (v >> 24));
        for (int m = 32; m >= 1; m >>= 1) body += __shfl_xor(body, m, 64);
        body = __builtin_amdgcn_readfirstlane(body);                // every lane has the sum: pos stays a scalar
        if (!oggchain_body_fits(left, nseg, body)) break;
        const uint32_t sno = (uint32_t)__builtin_amdgcn_readlane(hb, 14) | ((uint32_t)__builtin_amdgcn_readlane(hb, 15) << 8) |
                             ((uint32_t)__builtin_amdgcn_readlane(hb, 16) << 16) |
                             ((uint32_t)__builtin_amdgcn_readlane(hb, 17) << 24);
        const bool head = oggsel_is_head(flags, pos, begin);
        bool mark = false;
        if (oggsel_wants_mark(w, head, body)) {                     // the body fits and has 7 bytes
            uint32_t lo, hi;
            if (nseg <= 244) {
                // they are bytes nseg .. nseg + 6 of what the lanes hold: words nseg / 4 .. nseg / 4 + 2, lane 63 at most
                const int w0 = nseg >> 2, sh = (nseg & 3) * 8;
                const uint32_t a = __builtin_amdgcn_readlane(lw, w0), b = __builtin_amdgcn_readlane(lw, w0 + 1),
                               c = __builtin_amdgcn_readlane(lw, w0 + 2);
                lo = sh ? (a >> sh) | (b << (32 - sh)) : a;
                hi = sh ? (b >> sh) | (c << (32 - sh)) : b;
            } else {
                const int bb = lane < 7 ? h[27 + nseg + lane] : 0;  // a second round trip
                lo = (uint32_t)__builtin_amdgcn_readlane(bb, 0) | ((uint32_t)__builtin_amdgcn_readlane(bb, 1) << 8) |
                     ((uint32_t)__builtin_amdgcn_readlane(bb, 2) << 16) | ((uint32_t)__builtin_amdgcn_readlane(bb, 3) << 24);
                hi = (uint32_t)__builtin_amdgcn_readlane(bb, 4) | ((uint32_t)__builtin_amdgcn_readlane(bb, 5) << 8) |
                     ((uint32_t)__builtin_amdgcn_readlane(bb, 6) << 16);
            }
            mark = oggsel_is_mark(lo, hi);
        }
        const int len = 27 + nseg + body;
        if (oggsel_choose(w, head, sno, mark)) {
            oggsel_keep(w, pos, len);
            w.info.kept_pages++;
        } else {
            w.info.foreign_pages++;
            room_left = oggsel_flush(w, runs + slot, room, lane == 0);
        }
        pos += len;
    }
    if (room_left) {
        oggsel_stop(w, pos, end);
        oggsel_flush(w, runs + slot, room, lane == 0);
    }
    if (lane == 0) {
        info[f] = w.info;
        nruns[f] = w.nruns;
        kept[f] = w.info.kept_bytes;
    }
}

__global__ void __launch_bounds__(256) k_sel_scan(int nfiles, const long long *kept, long long *out_offsets, long long out_cap,
                                                  int *status)
{
    __shared__ long long wave_sum[4];
    block_scan_array<1>(nfiles, kept, out_offsets, out_offsets + nfiles, wave_sum);
    if (threadIdx.x == 0) *status = out_offsets[nfiles] > out_cap ? VBM_OGG_DEMUX_ECAP : 0;   // its own store
}

__global__ void __launch_bounds__(256) k_sel_copy(int nfiles, const uint8_t *data, const long long *off, const OggSelRun *runs,
                                                  const long long *nruns, const long long *out_offsets, uint8_t *out,
                                                  long long out_cap)
{
    const long long total = out_offsets[nfiles];
    if (total > out_cap) return;                    // the kept bytes do not fit: nothing is written
    long long d = (long long)blockIdx.x * kChunk;   // everything below is the same in every thread
    if (d >= total) return;                         // the grid is sized from the input
    const long long d1 = min(d + kChunk, total);
    int f = oggdmx_file_of_page(out_offsets, nfiles, d);
    long long fbase = out_offsets[f], nr = nruns[f];
    const OggSelRun *fr = runs + oggdmx_first_slot(off, f);
    long long r = oggsel_run_of(fr, nr, d - fbase);
    while (d < d1) {
        const OggSelRun R = fr[r];
        const long long within = d - fbase - R.dst;
        const long long n = min(R.len - within, d1 - d);
        vec_copy<256>(out + d, data + R.src + within, (int)n, threadIdx.x);
        d += n;
        if (within + n < R.len) break;              // the chunk ends inside this run
        r++;
        while (r == nr && f + 1 < nfiles) {         // the next file that keeps something
            f++;
            fbase = out_offsets[f], nr = nruns[f], r = 0;
            fr = runs + oggdmx_first_slot(off, f);
        }
        if (r == nr) break;                         // no run is left: d == total
    }
}

}  // namespace

// ---- host side (scaffold: twin_host.h) --------------------------------------------------------------------------

struct vbm_ogg_selector {
    bool host = false;
    int max_files = 0;
    long long max_bytes = 0, max_slots = 0;
    TwinMem mem;                         // owns the workspace
    long long *off = nullptr;            // [max_files + 1] the call's file offsets
    OggSelRun *runs = nullptr;           // [max_slots] the runs of every file, from the file's first slot on
    long long *nruns = nullptr;          // [max_files]
    long long *kept = nullptr;           // [max_files] kept bytes, what the scan reads
    int *status = nullptr;               // the status word of the last selection
    ArgStage stage;                      // device form: the file offsets go up through it, [max_files + 1]
};

namespace {

int create(vbm_ogg_selector **out, int max_files, long long max_bytes, bool host)
{
    if (!out || max_files < 1 || max_bytes < 0)
        return fail(VBM_EINVAL, "vbm_ogg_select_create: bad argument (max_files >= 1, max_bytes >= 0)");
    if (!host) {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n < 1) return fail(VBM_ENODEV, "vbm_ogg_select_create: no HIP device");
    }
    vbm_ogg_selector *m = new (std::nothrow) vbm_ogg_selector();
    if (!m) return fail(VBM_EFAULT, "vbm_ogg_select_create: out of memory");
    m->host = m->mem.host = host;
    m->max_files = max_files;
    m->max_bytes = max_bytes;
    m->max_slots = max_bytes / 27 + 1;
    const size_t F = (size_t)max_files;
    const char *who = "vbm_ogg_select";
    int rc = m->mem.get(m->off, F + 1, who);
    if (!rc) rc = m->mem.get(m->runs, (size_t)m->max_slots, who);
    if (!rc) rc = m->mem.get(m->nruns, F, who);
    if (!rc) rc = m->mem.get(m->kept, F, who);
    if (!rc) rc = m->mem.get(m->status, 1, who);
    if (!rc && !host) rc = m->stage.create((F + 1) * sizeof(long long), "vbm_ogg_select_create: staging");
    if (rc) {
        vbm_ogg_select_destroy(m);
        return rc;
    }
    *out = m;
    return VBM_OK;
}

int check_select(const vbm_ogg_selector *m, bool host, int nfiles, const uint8_t *data, const long long *off, const uint8_t *out,
                 long long out_cap, const long long *out_offsets, const vbm_ogg_select_info *info, const char *who)
{
    if (int rc = check_kind(m, host, who, "select")) return rc;
    if (nfiles < 0 || nfiles > m->max_files)
        return fail(VBM_EINVAL, std::string(who) + ": nfiles is negative or above max_files");
    if (!off || !out_offsets || (nfiles > 0 && !info)) return fail(VBM_EINVAL, std::string(who) + ": null pointer");
    if (out_cap < 0) return fail(VBM_EINVAL, std::string(who) + ": negative capacity");
    if (out_cap > 0 && !out) return fail(VBM_EINVAL, std::string(who) + ": null output");
    if (off[0] < 0) return fail(VBM_EINVAL, std::string(who) + ": negative file offset");
    for (int f = 0; f < nfiles; f++)
        if (off[f + 1] < off[f]) return fail(VBM_EINVAL, std::string(who) + ": file offsets decrease");
    if (off[nfiles] - off[0] > m->max_bytes)
        return fail(VBM_EINVAL, std::string(who) + ": the files span " + std::to_string(off[nfiles] - off[0]) +
                                    " bytes, above max_bytes = " + std::to_string(m->max_bytes));
    if (off[nfiles] > off[0] && !data) return fail(VBM_EINVAL, std::string(who) + ": null data");
    if (off[nfiles] > off[0] && out_cap > 0 && (uintptr_t)out < (uintptr_t)(data + off[nfiles]) &&
        (uintptr_t)(data + off[0]) < (uintptr_t)(out + out_cap))
        return fail(VBM_EINVAL, std::string(who) + ": the output overlaps the files (the selection is not done in place)");
    return VBM_OK;
}

}  // namespace

extern "C" int vbm_ogg_select_create(vbm_ogg_selector **sel, int max_files, long long max_bytes)
{
    return create(sel, max_files, max_bytes, false);
}

extern "C" int vbm_host_ogg_select_create(vbm_ogg_selector **sel, int max_files, long long max_bytes)
{
    return create(sel, max_files, max_bytes, true);
}

extern "C" void vbm_ogg_select_destroy(vbm_ogg_selector *m)
{
    if (!m) return;
    m->mem.free_all();
    m->stage.destroy();
    delete m;
}

extern "C" int vbm_ogg_select(vbm_ogg_selector *m, int nfiles, const uint8_t *d_data, const long long *file_offsets,
                              uint8_t *d_out, long long out_cap, long long *d_out_offsets, vbm_ogg_select_info *d_info,
                              void *stream)
{
    int rc = check_select(m, false, nfiles, d_data, file_offsets, d_out, out_cap, d_out_offsets, d_info, "vbm_ogg_select");
    if (rc) return rc;
    hipStream_t q = (hipStream_t)stream;
    const size_t off_bytes = ((size_t)nfiles + 1) * sizeof(long long);
    void *h_off;
    rc = m->stage.next(h_off, "vbm_ogg_select: hipEventSynchronize(stage)");
    if (rc) return rc;
    memcpy(h_off, file_offsets, off_bytes);
    rc = m->stage.send(m->off, off_bytes, q, "vbm_ogg_select: upload of the file offsets");
    if (rc) return rc;
    if (nfiles > 0)
        hipLaunchKernelGGL(k_sel_walk, dim3(nfiles), dim3(64), 0, q, d_data, m->off, m->runs, m->nruns, m->kept, d_info);
    hipLaunchKernelGGL(k_sel_scan, dim3(1), dim3(256), 0, q, nfiles, m->kept, d_out_offsets, out_cap, m->status);
    // the kept total is on the device alone: one block per chunk of the input, which is no less
    const long long blocks = (file_offsets[nfiles] - file_offsets[0] + kChunk - 1) / kChunk;
    if (blocks > 0)
        hipLaunchKernelGGL(k_sel_copy, dim3((unsigned)blocks), dim3(256), 0, q, nfiles, d_data, m->off, m->runs, m->nruns,
                           d_out_offsets, d_out, out_cap);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? VBM_OK : vbm_set_hip_error(e, "vbm_ogg_select: launch");
}

extern "C" int vbm_ogg_select_status(vbm_ogg_selector *m, int *status, void *stream)
{
    if (!m || !status) return fail(VBM_EINVAL, "vbm_ogg_select_status: null pointer");
    return read_status(m->host, m->status, status, stream, "vbm_ogg_select_status");
}

// ---- the same on the CPU: the functions of ogg_select.h, file after file, and a memcpy per run -------------------------
extern "C" int vbm_host_ogg_select(vbm_ogg_selector *m, int nfiles, const uint8_t *data, const long long *file_offsets,
                                   uint8_t *out, long long out_cap, long long *out_offsets, vbm_ogg_select_info *info)
{
    int rc = check_select(m, true, nfiles, data, file_offsets, out, out_cap, out_offsets, info, "vbm_host_ogg_select");
    if (rc) return rc;
    memcpy(m->off, file_offsets, ((size_t)nfiles + 1) * sizeof(long long));
    long long total = 0;
    for (int f = 0; f < nfiles; f++) {
        const long long slot = oggdmx_first_slot(m->off, f), room = oggdmx_first_slot(m->off, f + 1) - slot;
        out_offsets[f] = total;
        m->nruns[f] = oggsel_walk_file(data, m->off[f], m->off[f + 1], m->runs + slot, room, info[f]);
        total += info[f].kept_bytes;
    }
    out_offsets[nfiles] = total;
    if (total > out_cap) {
        *m->status = VBM_OGG_DEMUX_ECAP;
        return VBM_OK;
    }
    *m->status = 0;
    for (int f = 0; f < nfiles; f++) {
        const OggSelRun *fr = m->runs + oggdmx_first_slot(m->off, f);
        for (long long r = 0; r < m->nruns[f]; r++) memcpy(out + out_offsets[f] + fr[r].dst, data + fr[r].src, (size_t)fr[r].len);
    }
    return VBM_OK;
}
