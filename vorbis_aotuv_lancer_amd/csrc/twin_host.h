// Host-side scaffold of the container objects that come as a device form and a host twin (ogg_mux.hip, ogg_demux.hip,
// ogg_feed.hip, ogg_chain.hip, ogg_select.hip, ogg_cut.hip): the host CRC table, the error setter, the kind check, the owner of the object's memory, the pinned
// stage a call's host arguments go up through, and the read-back of a status word.  Everything here has internal
// linkage: each of those files gets its own copy and none exports a name.
#pragma once
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string>

#include "ogg_mux.h"
#include "vbm_internal.h"

namespace {

struct CrcTable {
    uint32_t t[256];
    CrcTable() { for (uint32_t i = 0; i < 256; i++) t[i] = oggmux_crc_entry(i); }
};

const CrcTable &crc_table()
{
    static const CrcTable c;
    return c;
}

int fail(int code, const std::string &msg)
{
    g_vbm_err = msg;
    return code;
}

// a host call needs the twin, a device call the device form; kind: "mux", "demuxer", "feed", "chain", "select", "cut"
template <class M> int check_kind(const M *m, bool host, const char *who, const char *kind)
{
    if (m && m->host == host) return VBM_OK;
    return fail(VBM_EINVAL, std::string(who) + ": needs a " + kind + " made by vbm_" + (host ? "host_" : "") + "ogg_" + kind + "_create");
}

// The memory of one object: device memory, or host memory (calloc) for the twin.  It remembers what it handed out, so
// that destroying a half-built object releases exactly what was got.
struct TwinMem {
    bool host = false;
    int n = 0;
    void *held[20] = {};

    // p = count zeroed elements (one at least); who: the object's name in the error text
    template <class T> int get(T *&p, size_t count, const char *who)
    {
        const size_t bytes = (count ? count : 1) * sizeof(T);
        if (n == 20) return fail(VBM_EFAULT, std::string(who) + ": too many buffers");
        void *v = nullptr;
        if (host) {
            v = calloc(bytes, 1);
            if (!v) return fail(VBM_EFAULT, std::string(who) + ": out of host memory");
            held[n++] = v;
        } else {
            hipError_t e = hipMalloc(&v, bytes);
            if (e != hipSuccess) return vbm_set_hip_error(e, (std::string(who) + ": hipMalloc").c_str());
            held[n++] = v;
            e = hipMemset(v, 0, bytes);
            if (e != hipSuccess) return vbm_set_hip_error(e, (std::string(who) + ": hipMemset").c_str());
        }
        p = (T *)v;
        return VBM_OK;
    }

    void free_all()
    {
        while (n > 0) {
            n--;
            if (host) free(held[n]);
            else (void)hipFree(held[n]);
        }
    }
};

// Two pinned slots for the host arguments of a call on a stream: the call after next reuses a slot, so the only wait
// is for the copy out of it two calls ago.
struct ArgStage {
    void *slot[2] = {};
    hipEvent_t ev[2] = {};
    int turn = 1;                // the slot of the last call

    int create(size_t bytes, const char *who)
    {
        for (int i = 0; i < 2; i++) {
            hipError_t e = hipHostMalloc(&slot[i], bytes, hipHostMallocDefault);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming);
            if (e != hipSuccess) return vbm_set_hip_error(e, who);
        }
        return VBM_OK;
    }

    // the next slot's host pointer, once the last copy out of it is done
    int next(void *&p, const char *who)
    {
        turn ^= 1;
        const hipError_t e = hipEventSynchronize(ev[turn]);
        if (e != hipSuccess) return vbm_set_hip_error(e, who);
        p = slot[turn];
        return VBM_OK;
    }

    // that slot -> dst on q
    int send(void *dst, size_t bytes, hipStream_t q, const char *who)
    {
        hipError_t e = hipMemcpyAsync(dst, slot[turn], bytes, hipMemcpyHostToDevice, q);
        if (e == hipSuccess) e = hipEventRecord(ev[turn], q);
        return e == hipSuccess ? VBM_OK : vbm_set_hip_error(e, who);
    }

    void destroy()
    {
        for (int i = 0; i < 2; i++) {
            if (slot[i]) (void)hipHostFree(slot[i]);
            if (ev[i]) (void)hipEventDestroy(ev[i]);
        }
    }
};

// *status = the status word of the last fill (device form: waits for `stream`)
int read_status(bool host, const int *word, int *status, void *stream, const char *who)
{
    if (host) {
        *status = *word;
        return VBM_OK;
    }
    hipError_t e = hipMemcpyAsync(status, word, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    return e == hipSuccess ? VBM_OK : vbm_set_hip_error(e, who);
}

}  // namespace
