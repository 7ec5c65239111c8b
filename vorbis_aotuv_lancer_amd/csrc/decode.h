// Vorbis I packet unpack, written once for the host (vbm_host_unpack_packet) and the device (decode_kernels.hip).
//
// Restates, per audio packet: vorbis_synthesis (reference lib/synthesis.c:25-91: packet type, mode, W/lW/nW),
// floor1_inverse1 (lib/floor1.c:976-1045: the Y list with prediction), the residue decode of mapping0_inverse
// (lib/mapping0.c:1324-1497: floor-used propagation over coupling pairs, res0/1/2_inverse lib/res0.c:643-830,
// vorbis_book_decodev* lib/codebook.c:518-640), and decode_packed_entry_number's end-of-packet rules.
//
// Packets come from outside the program.  Every read is bounded by the packet's byte count, and every value taken
// from the bitstream is range-checked before it indexes a table: codebook entries come out of the decoder below
// (always < entries), partition classes out of the residue's decode map (always < partitions), post counts and
// indices were bounded when the setup header was parsed (decode_setup.cpp).
#pragma once
#include <stdint.h>
#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define VBMD_HD __host__ __device__ inline
#else
#define VBMD_HD inline
#endif

enum {
    VBMD_MAXCH = 8,
    VBMD_POSTS = 65,          // VIF_POSIT + 2
    VBMD_MAXBOOKS = 256,
    VBMD_MAXCONF = 64,        // floors, residues, mappings, modes: 6-bit counts
    VBMD_MAXSTEPS = 256,      // coupling steps: 8-bit count
};

struct vbmd_book {
    int entries, dim, used, maxlen, tabn, maptype;
    uint32_t off_code;   // uint32 [used]: codewords, first bit at the MSB, sorted ascending (the reference's codelist)
    uint32_t off_entry;  // int32  [used]: entry number of each sorted codeword
    uint32_t off_len;    // uint8  [used]: length of each sorted codeword
    uint32_t off_tab;    // uint32 [1 << tabn]: sorted index + 1 of the codeword the next tabn bits start, 0 = longer
    uint32_t off_vals;   // float  [entries * dim]: dequantised vector of each entry (maptype 1, 2)
};

struct vbmd_floor {
    int partitions, mult, posts, quant_q, qbits;
    int partclass[32];
    int class_dim[16], class_subs[16], class_book[16], subbook[16][8];
    int postlist[VBMD_POSTS];
    int fwd[VBMD_POSTS];                 // post indices in ascending x (floor1_look's forward_index)
    int lo[VBMD_POSTS - 2], hi[VBMD_POSTS - 2];
};

struct vbmd_residue {
    int type, begin, end, grouping, partitions, groupbook, stages, partvals;
    int secondstages[64];
    int books[64][8];                    // -1: none
};

struct vbmd_mapping {
    int submaps, steps;
    unsigned char mag[VBMD_MAXSTEPS], ang[VBMD_MAXSTEPS];
    unsigned char mux[VBMD_MAXCH];
    unsigned char floorsub[16], ressub[16];
};

struct vbmd_setup {
    int channels, rate, blocksizes[2];
    int modes, modebits, books, floors, residues, maps;
    int mode_blockflag[VBMD_MAXCONF], mode_mapping[VBMD_MAXCONF];
    int max_classes;                     // bytes of partition-class scratch one packet needs (vbmd_unpack's cls)
    vbmd_mapping map[VBMD_MAXCONF];
    vbmd_floor floor[VBMD_MAXCONF];
    vbmd_residue res[VBMD_MAXCONF];
    vbmd_book book[VBMD_MAXBOOKS];
    uint32_t blob_bytes;                 // the book tables follow the struct (4-byte aligned offsets into the blob)
};

// ---- bit reader: oggpack_look / _read / _adv (LSb first).  pos > 8*bytes: a read ran past the end (sticky) ----------
struct vbmd_bits {
    const uint8_t *p;
    long bytes, pos;
};

VBMD_HD long vbmd_look(const vbmd_bits &b, int n)
{
    if (b.pos + n > 8 * b.bytes) return -1;
    if (n == 0) return 0;
    const long first = b.pos >> 3, last = (b.pos + n - 1) >> 3;
    uint64_t w = 0;
    for (long k = first; k <= last; k++) w |= (uint64_t)b.p[k] << (8 * (k - first));
    w >>= (b.pos & 7);
    return (long)(w & (n == 32 ? 0xffffffffull : ((1ull << n) - 1)));
}

VBMD_HD long vbmd_read(vbmd_bits &b, int n)
{
    const long v = vbmd_look(b, n);
    if (v < 0) { b.pos = 8 * b.bytes + 1; return -1; }
    b.pos += n;
    return v;
}

VBMD_HD uint32_t vbmd_brev32(uint32_t x)
{
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
    x = ((x >> 4) & 0x0f0f0f0fu) | ((x & 0x0f0f0f0fu) << 4);
    x = ((x >> 8) & 0x00ff00ffu) | ((x & 0x00ff00ffu) << 8);
    return (x >> 16) | (x << 16);
}

VBMD_HD int vbmd_ilog(unsigned v)
{
    int r = 0;
    while (v) { r++; v >>= 1; }
    return r;
}

// vorbis_book_decode -> entry number (< entries), or -1.  A codeword decodes only if all its bits lie in the packet;
// otherwise the remaining bits are consumed and -1 returned (decode_packed_entry_number).
VBMD_HD int vbmd_decode(const vbmd_book &bk, const uint8_t *blob, vbmd_bits &b)
{
    if (bk.used <= 0) return -1;
    const long avail = 8 * b.bytes - b.pos;
    if (avail <= 0) return -1;
    const int rd = bk.maxlen < avail ? bk.maxlen : (int)avail;
    const uint32_t lok = (uint32_t)vbmd_look(b, rd);
    const uint32_t *code = (const uint32_t *)(blob + bk.off_code);
    const int *entry = (const int *)(blob + bk.off_entry);
    const uint8_t *len = blob + bk.off_len;
    if (rd >= bk.tabn) {
        const int t = (int)((const uint32_t *)(blob + bk.off_tab))[lok & ((1u << bk.tabn) - 1)];
        if (t > 0) { b.pos += len[t - 1]; return entry[t - 1]; }
    }
    const uint32_t test = vbmd_brev32(lok);
    int lo = 0, hi = bk.used;
    while (hi - lo > 1) {
        const int p = (hi - lo) >> 1;
        if (code[lo + p] > test) hi -= p;
        else lo += p;
    }
    if (len[lo] <= rd) { b.pos += len[lo]; return entry[lo]; }
    b.pos += rd;
    return -1;
}

// ---- floor 1: floor1_inverse1 -------------------------------------------------------------------------------------
// fit[] gets the unwrapped Y values (bit 15: predicted, not coded); returns 0 at end of packet (channel unused)
VBMD_HD int vbmd_render_point(int x0, int x1, int y0, int y1, int x)
{
    y0 &= 0x7fff;
    y1 &= 0x7fff;
    const int dy = y1 - y0, adx = x1 - x0;
    const int ady = dy < 0 ? -dy : dy;
    const int off = ady * (x - x0) / adx;
    return dy < 0 ? y0 - off : y0 + off;
}

VBMD_HD int vbmd_floor1_inverse1(const vbmd_setup &s, const uint8_t *blob, const vbmd_floor &f, vbmd_bits &b, int *fit)
{
    if (vbmd_read(b, 1) != 1) return 0;
    fit[0] = (int)vbmd_read(b, f.qbits);
    fit[1] = (int)vbmd_read(b, f.qbits);
    // The reference does not test these two reads (lib/floor1.c:988-989); a later book read catches the end of the
    // packet for it, unless the floor has no book to read (no partitions, or classes without books), where it
    // goes on with Y = -1.  The specification (7.2.3) marks the channel unused, and so does this.  The PCM is the
    // same either way: at the end of the packet no residue is left to decode.
    if (fit[1] < 0) return 0;
    for (int i = 0, j = 2; i < f.partitions; i++) {
        const int cls = f.partclass[i];
        const int cdim = f.class_dim[cls], csubbits = f.class_subs[cls], csub = 1 << csubbits;
        int cval = 0;
        if (csubbits) {
            cval = vbmd_decode(s.book[f.class_book[cls]], blob, b);
            if (cval == -1) return 0;
        }
        for (int k = 0; k < cdim; k++) {
            const int book = f.subbook[cls][cval & (csub - 1)];
            cval >>= csubbits;
            if (book >= 0) {
                if ((fit[j + k] = vbmd_decode(s.book[book], blob, b)) == -1) return 0;
            } else {
                fit[j + k] = 0;
            }
        }
        j += cdim;
    }
    for (int i = 2; i < f.posts; i++) {
        const int lo = f.lo[i - 2], hi = f.hi[i - 2];
        const int predicted = vbmd_render_point(f.postlist[lo], f.postlist[hi], fit[lo], fit[hi], f.postlist[i]);
        const int hiroom = f.quant_q - predicted, loroom = predicted;
        const int room = (hiroom < loroom ? hiroom : loroom) << 1;
        int val = fit[i];
        if (val) {
            if (val >= room) {
                if (hiroom > loroom) val = val - loroom;
                else val = -1 - (val - hiroom);
            } else {
                if (val & 1) val = -((val + 1) >> 1);
                else val >>= 1;
            }
            fit[i] = (val + predicted) & 0x7fff;
            fit[lo] &= 0x7fff;
            fit[hi] &= 0x7fff;
        } else {
            fit[i] = predicted | 0x8000;
        }
    }
    return 1;
}

// ---- residue: vorbis_book_decodevs_add / decodev_add / decodevv_add ------------------------------------------------
VBMD_HD int vbmd_decodevs_add(const vbmd_book &bk, const uint8_t *blob, float *a, vbmd_bits &b, int n)
{
    if (bk.used <= 0) return 0;
    const int step = n / bk.dim;
    // the reference decodes all `step` entries before it adds any: decode once to find out whether all are there,
    // then again from the same position, adding (each a[] element receives exactly one term, so the order is free)
    const long start = b.pos;
    for (int i = 0; i < step; i++)
        if (vbmd_decode(bk, blob, b) == -1) return -1;
    b.pos = start;
    const float *vals = (const float *)(blob + bk.off_vals);
    for (int j = 0; j < step; j++) {
        const int e = vbmd_decode(bk, blob, b);
        for (int i = 0, o = 0; i < bk.dim; i++, o += step)
            if (o + j < n) a[o + j] += vals[(long)e * bk.dim + i];
    }
    return 0;
}

VBMD_HD int vbmd_decodev_add(const vbmd_book &bk, const uint8_t *blob, float *a, vbmd_bits &b, int n)
{
    if (bk.used <= 0) return 0;
    const float *vals = (const float *)(blob + bk.off_vals);
    for (int i = 0; i < n;) {
        const int e = vbmd_decode(bk, blob, b);
        if (e == -1) return -1;
        const float *t = vals + (long)e * bk.dim;
        for (int j = 0; i < n && j < bk.dim;) a[i++] += t[j++];
    }
    return 0;
}

// a[c] = res + chan[c] * stride
VBMD_HD int vbmd_decodevv_add(const vbmd_book &bk, const uint8_t *blob, float *res, long stride, const int *chan,
                              long offset, int ch, vbmd_bits &b, int n)
{
    if (bk.used <= 0) return 0;
    const float *vals = (const float *)(blob + bk.off_vals);
    const long m = (offset + n) / ch;
    int chptr = 0;
    for (long i = offset / ch; i < m;) {
        const int e = vbmd_decode(bk, blob, b);
        if (e == -1) return -1;
        const float *t = vals + (long)e * bk.dim;
        for (int j = 0; i < m && j < bk.dim; j++) {
            res[chan[chptr++] * stride + i] += t[j];
            if (chptr == ch) { chptr = 0; i++; }
        }
    }
    return 0;
}

// _01inverse / res2_inverse over the channels chan[0..nch) of one submap.  n = blocksize/2.
// cls: scratch of s.max_classes bytes (partition class of every partition, kept from stage 0 for the later stages)
VBMD_HD void vbmd_residue_inverse(const vbmd_setup &s, const uint8_t *blob, const vbmd_residue &r, vbmd_bits &b,
                                  float *res, long stride, const int *chan, int nch, int n, uint8_t *cls)
{
    const vbmd_book &pb = s.book[r.groupbook];
    const int ppw = pb.dim;
    const int nvec = (r.type == 2) ? 1 : nch;
    const int max = (r.type == 2) ? n * nch : n;
    const int end = r.end < max ? r.end : max;
    const int len = end - r.begin;
    if (len <= 0 || nch <= 0) return;
    const int partvals = len / r.grouping;
    for (int st = 0; st < r.stages; st++) {
        for (int i = 0; i < partvals;) {
            if (st == 0) {
                for (int j = 0; j < nvec; j++) {
                    const int temp = vbmd_decode(pb, blob, b);
                    if (temp == -1 || temp >= r.partvals) return;
                    // decodemap: the ppw base-`partitions` digits of temp, most significant first
                    int mult = r.partvals / r.partitions, val = temp;
                    for (int k = 0; k < ppw; k++) {
                        const int deco = val / mult;
                        val -= deco * mult;
                        mult /= r.partitions;
                        if (i + k < partvals) cls[(long)j * partvals + i + k] = (uint8_t)deco;
                    }
                }
            }
            for (int k = 0; k < ppw && i < partvals; k++, i++) {
                const long offset = r.begin + (long)i * r.grouping;
                for (int j = 0; j < nvec; j++) {
                    const int c = cls[(long)j * partvals + i];
                    if (!(r.secondstages[c] & (1 << st))) continue;
                    const int book = r.books[c][st];
                    if (book < 0) continue;
                    int rc;
                    if (r.type == 2)
                        rc = vbmd_decodevv_add(s.book[book], blob, res, stride, chan, offset, nch, b, r.grouping);
                    else if (r.type == 1)
                        rc = vbmd_decodev_add(s.book[book], blob, res + chan[j] * stride + offset, b, r.grouping);
                    else
                        rc = vbmd_decodevs_add(s.book[book], blob, res + chan[j] * stride + offset, b, r.grouping);
                    if (rc == -1) return;
                }
            }
        }
    }
}

// ---- one packet ----------------------------------------------------------------------------------------------------
// The packet's header bits (vorbis_synthesis, lib/synthesis.c:25-91): packet type, mode, W, lW, nW.  Returns 0,
// VBM_ENOTAUDIO (-135) or VBM_EBADPACKET (-136).  Nothing after them can make a packet fail, so this decides the
// status of vbmd_unpack, and the host index (vbmd_index_stream) reads only this.
VBMD_HD int vbmd_head(const vbmd_setup &s, vbmd_bits &b, int &mode, int &W, int &lW, int &nW)
{
    if (vbmd_read(b, 1) != 0) return -135;
    mode = (int)vbmd_read(b, s.modebits);
    if (mode < 0 || mode >= s.modes) return -136;
    W = s.mode_blockflag[mode];
    lW = 0;
    nW = 0;
    if (W) {
        lW = (int)vbmd_read(b, 1);
        nW = (int)vbmd_read(b, 1);
        if (nW == -1) return -136;
    }
    return 0;
}

// vorbis_synthesis_blockin's bookkeeping (lib/block.c:1050-1161) for a valid packet of block size W after one of
// block size lW (-1: the stream's first): the part of the packet's output that becomes final, [begin, end), and the
// stream's sample count sc and granulepos gp (-1: none yet), advanced by the packet's granulepos vgp (-1: none) and
// its end-of-stream flag.  One definition for k_overlap, k_run_plan and the host index (vbmd_index_stream).
// HS: the reference's halfrate_flag.  begin / end are output samples (half as many at HS = 1); sc, gp and vgp stay
// full-rate, so a trim of `extra` full-rate samples, clamped to twice what the packet returns, takes extra >> 1
// output samples.  At HS = 0 every shift is by zero.
template <int HS = 0>
VBMD_HD void vbmd_blockin(const int *blocksizes, int lW, int W, long long vgp, int eof, long long &sc, long long &gp,
                          long &begin, long &end)
{
    begin = 0;
    end = 0;
    if (lW >= 0) end = ((blocksizes[lW] >> 2) + (blocksizes[W] >> 2)) >> HS;
    const long long step = (lW >= 0 ? (blocksizes[lW] >> 2) : 0) + (blocksizes[W] >> 2);
    sc = (sc == -1) ? 0 : sc + step;
    if (gp == -1) {
        if (vgp != -1) {
            gp = vgp;
            if (sc > gp) {
                long long extra = sc - vgp;
                if (extra < 0) extra = 0;
                if (eof) {
                    if (extra > (long long)(end - begin) << HS) extra = (long long)(end - begin) << HS;
                    end -= extra >> HS;
                } else {
                    begin += extra >> HS;
                    if (begin > end) begin = end;
                }
            }
        }
    } else {
        gp += step;
        if (vgp != -1 && gp != vgp) {
            if (gp > vgp) {
                long long extra = gp - vgp;
                if (extra && eof) {
                    if (extra > (long long)(end - begin) << HS) extra = (long long)(end - begin) << HS;
                    if (extra < 0) extra = 0;
                    end -= extra >> HS;
                }
            }
            gp = vgp;
        }
    }
}

// Returns vbmd_head's status.
//   info[4]      mode, W, lW, nW
//   fit          [channels][VBMD_POSTS] floor Y values (valid where bit 0 of flags is set)
//   flags        [channels] bit 0: the channel's floor is coded, bit 1: nonzero after the coupling propagation
//   res          [channels][stride] residue before inverse coupling; must be zero on entry (bins < blocksize/2 used)
//   cls          partition-class scratch, s.max_classes bytes
// Copy: one instantiation per kernel that calls it (k_unpack the default, k_unpack_csr 1, k_unpack_rows 2, the mixed
// forms of the first two 3 and 4), so that
// each has a single call site and is inlined as it was with one caller, instead of becoming a shared out-of-line
// function.
template <int Copy = 0>
VBMD_HD int vbmd_unpack(const vbmd_setup &s, const uint8_t *blob, const uint8_t *pkt, long bytes, int *info, int *fit,
                        int *flags, float *res, long stride, uint8_t *cls)
{
    vbmd_bits b = {pkt, bytes < 0 ? 0 : bytes, 0};
    info[0] = info[1] = info[2] = info[3] = 0;
    for (int c = 0; c < s.channels; c++) flags[c] = 0;
    int mode, W, lW, nW;
    const int head = vbmd_head(s, b, mode, W, lW, nW);
    if (head) return head;
    info[0] = mode;
    info[1] = W;
    info[2] = lW;
    info[3] = nW;
    const vbmd_mapping &m = s.map[s.mode_mapping[mode]];
    const int n = s.blocksizes[W] >> 1;
    int nonzero[VBMD_MAXCH];
    for (int c = 0; c < s.channels; c++) {
        const vbmd_floor &f = s.floor[m.floorsub[m.mux[c]]];
        nonzero[c] = vbmd_floor1_inverse1(s, blob, f, b, fit + c * VBMD_POSTS);
        flags[c] = nonzero[c];
    }
    for (int i = 0; i < m.steps; i++)
        if (nonzero[m.mag[i]] || nonzero[m.ang[i]]) nonzero[m.mag[i]] = nonzero[m.ang[i]] = 1;
    for (int c = 0; c < s.channels; c++) flags[c] |= nonzero[c] << 1;
    for (int sm = 0; sm < m.submaps; sm++) {
        const vbmd_residue &r = s.res[m.ressub[sm]];
        int chan[VBMD_MAXCH], nch = 0, any = 0;
        for (int c = 0; c < s.channels; c++) {
            if (m.mux[c] != sm) continue;
            if (r.type == 2) { chan[nch++] = c; any |= nonzero[c]; }   // res2: every channel of the bundle
            else if (nonzero[c]) chan[nch++] = c;                      // res0/1: the nonzero ones only
        }
        if (r.type == 2 && !any) continue;
        vbmd_residue_inverse(s, blob, r, b, res, stride, chan, nch, n, cls);
    }
    return 0;
}
