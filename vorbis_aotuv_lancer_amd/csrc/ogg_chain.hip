// The links of chained Ogg files, found on the device for many files per call (rule and workspace: ogg_chain.h), the host
// twin, and the C ABI over both (include/vorbis_mi355x.h, "Ogg chains"; host scaffold: twin_host.h).
//
//   k_chain_walk        one wavefront per file, page after page.  Per page every lane loads one header byte and four
//                       lacing bytes, each known to lie in front of the file's end, in one round trip; a wave reduction
//                       gives the body length, so the page's place, length and flag are uniform over the wavefront and
//                       lane 0 records a link start
//   k_chain_scan_links  one block, four files per thread: exclusive scan of the link counts -> d_file_links
//   k_chain_emit        the capacity check, then one thread per link: the dense offsets, and the closing entry
#include <hip/hip_runtime.h>
#include <string.h>
#include <new>
#include <string>

#include "ogg_chain.h"
#include "twin_host.h"

namespace {

constexpr int kEmitBlocks = 2048;  // most blocks k_chain_emit is launched with

// ---- kernels ---------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(64) k_chain_walk(const uint8_t *data, const long long *off, long long *starts,
                                                   long long *nlinks)
{
    const int f = blockIdx.x, lane = threadIdx.x;
    const long long begin = off[f], end = off[f + 1];
    const long long slot = oggdmx_first_slot(off, f), room = oggdmx_first_slot(off, f + 1) - slot;
    long long pos = begin, extra = 0;               // the same in every lane, as is every exit below
    for (;;) {
        const long long left = end - pos;
        if (left < 27) break;
        const uint8_t *h = data + pos;
        // the round trip: header byte `lane`, and lacing values 4 * lane .. 4 * lane + 3 if the file goes on that far
        // (past nseg they are body bytes of this file, and are masked below)
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
        if (oggchain_starts_link(flags, pos, begin)) {
            if (extra >= room) break;                               // cannot happen (ogg_chain.h): second line of defence
            if (lane == 0) starts[slot + extra] = pos;
            extra++;
        }
        pos += 27 + nseg + body;
    }
    if (lane == 0) nlinks[f] = 1 + extra;
}

__global__ void __launch_bounds__(256) k_chain_scan_links(int nfiles, const long long *nlinks, long long *file_links)
{
    __shared__ long long wave_sum[4];
    block_scan_array<1>(nfiles, nlinks, file_links, file_links + nfiles, wave_sum);
}

__global__ void __launch_bounds__(256) k_chain_emit(int nfiles, const long long *off, const long long *file_links,
                                                    const long long *starts, long long *link_offsets, long long link_cap,
                                                    int *status)
{
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    const long long total = file_links[nfiles];
    if (total > link_cap) {
        if (first) *status = VBM_OGG_DEMUX_ECAP;    // the links do not fit: nothing is written
        return;
    }
    if (first) {
        *status = 0;
        link_offsets[total] = off[nfiles];
    }
    const long long step = (long long)gridDim.x * 256;
    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < total; j += step)
        link_offsets[j] = oggchain_link_start(off, file_links, starts, nfiles, j);
}

}  // namespace

// ---- host side (scaffold: twin_host.h) --------------------------------------------------------------------------

struct vbm_ogg_chain {
    bool host = false;
    int max_files = 0;
    long long max_bytes = 0, max_slots = 0;
    TwinMem mem;                         // owns the workspace
    long long *off = nullptr;            // [max_files + 1] the call's file offsets
    long long *starts = nullptr;         // [max_slots] the starts of every file's links after its first
    long long *nlinks = nullptr;         // [max_files]
    int *status = nullptr;               // the status word of the last split
    ArgStage stage;                      // device form: the file offsets go up through it, [max_files + 1]
};

namespace {

int create(vbm_ogg_chain **out, int max_files, long long max_bytes, bool host)
{
    if (!out || max_files < 1 || max_bytes < 0)
        return fail(VBM_EINVAL, "vbm_ogg_chain_create: bad argument (max_files >= 1, max_bytes >= 0)");
    if (!host) {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n < 1) return fail(VBM_ENODEV, "vbm_ogg_chain_create: no HIP device");
    }
    vbm_ogg_chain *m = new (std::nothrow) vbm_ogg_chain();
    if (!m) return fail(VBM_EFAULT, "vbm_ogg_chain_create: out of memory");
    m->host = m->mem.host = host;
    m->max_files = max_files;
    m->max_bytes = max_bytes;
    m->max_slots = max_bytes / 27 + 1;
    const size_t F = (size_t)max_files;
    const char *who = "vbm_ogg_chain";
    int rc = m->mem.get(m->off, F + 1, who);
    if (!rc) rc = m->mem.get(m->starts, (size_t)m->max_slots, who);
    if (!rc) rc = m->mem.get(m->nlinks, F, who);
    if (!rc) rc = m->mem.get(m->status, 1, who);
    if (!rc && !host) rc = m->stage.create((F + 1) * sizeof(long long), "vbm_ogg_chain_create: staging");
    if (rc) {
        vbm_ogg_chain_destroy(m);
        return rc;
    }
    *out = m;
    return VBM_OK;
}

int check_split(const vbm_ogg_chain *m, bool host, int nfiles, const uint8_t *data, const long long *off,
                const long long *file_links, const long long *link_offsets, long long link_cap, const char *who)
{
    if (int rc = check_kind(m, host, who, "chain")) return rc;
    if (nfiles < 0 || nfiles > m->max_files)
        return fail(VBM_EINVAL, std::string(who) + ": nfiles is negative or above max_files");
    if (!off || !file_links || !link_offsets) return fail(VBM_EINVAL, std::string(who) + ": null pointer");
    if (link_cap < 0) return fail(VBM_EINVAL, std::string(who) + ": negative capacity");
    if (off[0] < 0) return fail(VBM_EINVAL, std::string(who) + ": negative file offset");
    for (int f = 0; f < nfiles; f++)
        if (off[f + 1] < off[f]) return fail(VBM_EINVAL, std::string(who) + ": file offsets decrease");
    if (off[nfiles] - off[0] > m->max_bytes)
        return fail(VBM_EINVAL, std::string(who) + ": the files span " + std::to_string(off[nfiles] - off[0]) +
                                    " bytes, above max_bytes = " + std::to_string(m->max_bytes));
    if (off[nfiles] > off[0] && !data) return fail(VBM_EINVAL, std::string(who) + ": null data");
    return VBM_OK;
}

}  // namespace

extern "C" int vbm_ogg_chain_create(vbm_ogg_chain **ch, int max_files, long long max_bytes)
{
    return create(ch, max_files, max_bytes, false);
}

extern "C" int vbm_host_ogg_chain_create(vbm_ogg_chain **ch, int max_files, long long max_bytes)
{
    return create(ch, max_files, max_bytes, true);
}

extern "C" void vbm_ogg_chain_destroy(vbm_ogg_chain *m)
{
    if (!m) return;
    m->mem.free_all();
    m->stage.destroy();
    delete m;
}

extern "C" int vbm_ogg_chain_split(vbm_ogg_chain *m, int nfiles, const uint8_t *d_data, const long long *file_offsets,
                                   long long *d_file_links, long long *d_link_offsets, long long link_cap, void *stream)
{
    int rc = check_split(m, false, nfiles, d_data, file_offsets, d_file_links, d_link_offsets, link_cap, "vbm_ogg_chain_split");
    if (rc) return rc;
    hipStream_t q = (hipStream_t)stream;
    const size_t off_bytes = ((size_t)nfiles + 1) * sizeof(long long);
    void *h_off;
    rc = m->stage.next(h_off, "vbm_ogg_chain_split: hipEventSynchronize(stage)");
    if (rc) return rc;
    memcpy(h_off, file_offsets, off_bytes);
    rc = m->stage.send(m->off, off_bytes, q, "vbm_ogg_chain_split: upload of the file offsets");
    if (rc) return rc;
    if (nfiles > 0)
        hipLaunchKernelGGL(k_chain_walk, dim3(nfiles), dim3(64), 0, q, d_data, m->off, m->starts, m->nlinks);
    hipLaunchKernelGGL(k_chain_scan_links, dim3(1), dim3(256), 0, q, nfiles, m->nlinks, d_file_links);
    // a file has one link and at most one more per page slot
    const long long most = nfiles + (file_offsets[nfiles] - file_offsets[0]) / 27, blocks = (most + 255) / 256;
    hipLaunchKernelGGL(k_chain_emit, dim3((unsigned)(blocks < 1 ? 1 : blocks < kEmitBlocks ? blocks : kEmitBlocks)), dim3(256), 0,
                       q, nfiles, m->off, d_file_links, m->starts, d_link_offsets, link_cap, m->status);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? VBM_OK : vbm_set_hip_error(e, "vbm_ogg_chain_split: launch");
}

extern "C" int vbm_ogg_chain_status(vbm_ogg_chain *m, int *status, void *stream)
{
    if (!m || !status) return fail(VBM_EINVAL, "vbm_ogg_chain_status: null pointer");
    return read_status(m->host, m->status, status, stream, "vbm_ogg_chain_status");
}

// ---- the same on the CPU: the functions of ogg_chain.h, file after file and page after page ---------------------------
extern "C" int vbm_host_ogg_chain_split(vbm_ogg_chain *m, int nfiles, const uint8_t *data, const long long *file_offsets,
                                        long long *file_links, long long *link_offsets, long long link_cap)
{
    int rc = check_split(m, true, nfiles, data, file_offsets, file_links, link_offsets, link_cap, "vbm_host_ogg_chain_split");
    if (rc) return rc;
    memcpy(m->off, file_offsets, ((size_t)nfiles + 1) * sizeof(long long));
    long long total = 0;
    for (int f = 0; f < nfiles; f++) {
        const long long slot = oggdmx_first_slot(m->off, f), room = oggdmx_first_slot(m->off, f + 1) - slot;
        file_links[f] = total;
        total += oggchain_walk_file(data, m->off[f], m->off[f + 1], m->starts + slot, room);
    }
    file_links[nfiles] = total;
    if (total > link_cap) {
        *m->status = VBM_OGG_DEMUX_ECAP;
        return VBM_OK;
    }
    *m->status = 0;
    for (long long j = 0; j < total; j++) link_offsets[j] = oggchain_link_start(m->off, file_links, m->starts, nfiles, j);
    link_offsets[total] = m->off[nfiles];
    return VBM_OK;
}
