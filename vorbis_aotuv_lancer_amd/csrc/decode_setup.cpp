// Decode setup (host only): the three Vorbis header packets -> the tables vbmd_unpack (decode.h) reads.
//
// Restates vorbis_synthesis_headerin (reference lib/info.c:237-498) with vorbis_staticbook_unpack
// (lib/codebook.c:277-400), floor1_unpack / floor1_look (lib/floor1.c:119-182, :184-230), res0_unpack / res0_look
// (lib/res0.c:191-300) and mapping0_unpack (lib/mapping0.c:95-), and the decode tables of vorbis_book_init_decode
// (_make_words, _book_unquantize: lib/sharedbook.c:85-459).  Error codes are the reference's (OV_*); what this
// decoder does not implement (floor 0, block sizes outside 256..4096, more than 8 channels) is VBM_EIMPL.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <dlfcn.h>
#include <string>
#include <vector>

#include "decode.h"
#include "decode_setup.h"
#include "vbm_internal.h"
#include "vorbis_mi355x.h"
#include "vpk.h"

namespace {

struct Book {            // static codebook as unpacked
    int dim = 0, entries = 0, maptype = 0, q_quant = 0, q_seq = 0;
    long q_min = 0, q_delta = 0;
    std::vector<int> len;
    std::vector<long> quant;
};

float float32_unpack(long val)          // lib/sharedbook.c:_float32_unpack
{
    double mant = val & 0x1fffff;
    const long sign = val & 0x80000000;
    long exp = (val & 0x7fe00000L) >> 21;
    if (sign) mant = -mant;
    exp = exp - (21 - 1) - 768;
    if (exp > 63) exp = 63;
    if (exp < -63) exp = -63;
    return (float)ldexp(mant, (int)exp);
}

// the greatest v with v^dim <= entries (_book_maptype1_quantvals, by integer means)
long maptype1_quantvals(long entries, int dim)
{
    if (entries < 1 || dim < 1) return 0;
    long v = (long)floor(pow((double)entries, 1.0 / dim));
    if (v < 1) v = 1;
    auto fits = [&](long x) {
        long acc = 1;
        for (int i = 0; i < dim; i++) {
            if (acc > entries / x) return false;
            acc *= x;
        }
        return acc <= entries;
    };
    while (v > 1 && !fits(v)) v--;
    while (fits(v + 1)) v++;
    return v;
}

int unpack_book(vbmd_bits &b, Book &s)
{
    if (vbmd_read(b, 24) != 0x564342) return -1;
    s.dim = (int)vbmd_read(b, 16);
    s.entries = (int)vbmd_read(b, 24);
    if (s.entries == -1) return -1;
    if (vbmd_ilog((unsigned)s.dim) + vbmd_ilog((unsigned)s.entries) > 24) return -1;
    s.len.assign(s.entries, 0);
    const long left = b.bytes - (b.pos + 7) / 8;
    switch ((int)vbmd_read(b, 1)) {
    case 0: {
        const long unused = vbmd_read(b, 1);
        if ((s.entries * (unused ? 1 : 5) + 7) >> 3 > left) return -1;
        for (int i = 0; i < s.entries; i++) {
            if (unused) {
                if (vbmd_read(b, 1)) {
                    const long num = vbmd_read(b, 5);
                    if (num == -1) return -1;
                    s.len[i] = (int)num + 1;
                } else {
                    s.len[i] = 0;
                }
            } else {
                const long num = vbmd_read(b, 5);
                if (num == -1) return -1;
                s.len[i] = (int)num + 1;
            }
        }
        break;
    }
    case 1: {
        long length = vbmd_read(b, 5) + 1;
        if (length == 0) return -1;
        for (int i = 0; i < s.entries;) {
            const long num = vbmd_read(b, vbmd_ilog((unsigned)(s.entries - i)));
            if (num == -1) return -1;
            if (length > 32 || num > s.entries - i || (num > 0 && (num - 1) >> (length - 1) > 1)) return -1;
            for (long j = 0; j < num; j++, i++) s.len[i] = (int)length;
            length++;
        }
        break;
    }
    default:
        return -1;
    }
    switch ((s.maptype = (int)vbmd_read(b, 4))) {
    case 0:
        break;
    case 1:
    case 2: {
        s.q_min = vbmd_read(b, 32);
        s.q_delta = vbmd_read(b, 32);
        s.q_quant = (int)vbmd_read(b, 4) + 1;
        s.q_seq = (int)vbmd_read(b, 1);
        if (s.q_seq == -1) return -1;
        const long qv = s.maptype == 1 ? (s.dim == 0 ? 0 : maptype1_quantvals(s.entries, s.dim)) : (long)s.entries * s.dim;
        if ((qv * s.q_quant + 7) >> 3 > b.bytes - (b.pos + 7) / 8) return -1;
        s.quant.resize(qv);
        for (long i = 0; i < qv; i++) s.quant[i] = vbmd_read(b, s.q_quant);
        if (qv && s.quant[qv - 1] == -1) return -1;
        break;
    }
    default:
        return -1;
    }
    return 0;
}

// _make_words: MSB-first canonical codewords of the used entries; empty on an over- or underpopulated tree
bool make_words(const std::vector<int> &l, std::vector<uint32_t> &r)
{
    uint32_t marker[33] = {};
    r.clear();
    for (size_t i = 0; i < l.size(); i++) {
        const int length = l[i];
        if (length <= 0) continue;
        uint32_t entry = marker[length];
        if (length < 32 && (entry >> length)) return false;
        r.push_back(entry);
        for (int j = length; j > 0; j--) {
            if (marker[j] & 1) {
                if (j == 1) marker[1]++;
                else marker[j] = marker[j - 1] << 1;
                break;
            }
            marker[j]++;
        }
        for (int j = length + 1; j < 33; j++) {
            if ((marker[j] >> 1) == entry) {
                entry = marker[j];
                marker[j] = marker[j - 1] << 1;
            } else {
                break;
            }
        }
    }
    if (!(r.size() == 1 && marker[2] == 2))
        for (int i = 1; i < 33; i++)
            if (marker[i] & (0xffffffffu >> (32 - i))) return false;
    return true;
}

struct Blob {
    std::vector<uint8_t> d;
    template <typename T>
    uint32_t put(const T *p, size_t n)
    {
        while (d.size() % 4) d.push_back(0);
        const uint32_t off = (uint32_t)d.size();
        d.resize(d.size() + n * sizeof(T));
        if (n) memcpy(d.data() + off, p, n * sizeof(T));
        return off;
    }
};

// vorbis_book_init_decode + _book_unquantize
int build_book(const Book &s, vbmd_book &o, Blob &blob)
{
    std::vector<uint32_t> words;
    if (!make_words(s.len, words)) return -1;
    o.entries = s.entries;
    o.dim = s.dim;
    o.maptype = s.maptype;
    o.used = (int)words.size();
    struct Cw { uint32_t code; int entry, len; };
    std::vector<Cw> cw;
    int maxlen = 0;
    for (int i = 0, k = 0; i < s.entries; i++) {
        if (s.len[i] <= 0) continue;
        const int L = s.len[i];
        cw.push_back({L == 32 ? words[k] : (words[k] << (32 - L)), i, L});
        maxlen = std::max(maxlen, L);
        k++;
    }
    std::sort(cw.begin(), cw.end(), [](const Cw &a, const Cw &b) { return a.code < b.code; });
    o.maxlen = maxlen;
    o.tabn = std::max(1, std::min(8, maxlen));
    std::vector<uint32_t> code(cw.size());
    std::vector<int> ent(cw.size());
    std::vector<uint8_t> len(cw.size());
    for (size_t i = 0; i < cw.size(); i++) { code[i] = cw[i].code; ent[i] = cw[i].entry; len[i] = (uint8_t)cw[i].len; }
    // first-level table, indexed by the next tabn stream bits (first bit = bit 0)
    std::vector<uint32_t> tab((size_t)1 << o.tabn, 0);
    for (size_t i = 0; i < cw.size(); i++) {
        if (cw[i].len > o.tabn) continue;
        const uint32_t msb = cw[i].code >> (32 - o.tabn);          // codeword left-aligned in tabn bits
        const uint32_t span = 1u << (o.tabn - cw[i].len);
        for (uint32_t t = 0; t < span; t++) {
            const uint32_t v = msb | t;
            uint32_t rev = 0;                                        // stream order: first bit at bit 0
            for (int j = 0; j < o.tabn; j++) rev |= ((v >> (o.tabn - 1 - j)) & 1u) << j;
            tab[rev] = (uint32_t)(i + 1);
        }
    }
    // a single-entry book of length 1 decodes either bit to its entry (vorbis_book_init_decode's special case)
    if (cw.size() == 1 && cw[0].len == 1) tab.assign(tab.size(), 1);
    o.off_code = blob.put(code.data(), code.size());
    o.off_entry = blob.put(ent.data(), ent.size());
    o.off_len = blob.put(len.data(), len.size());
    o.off_tab = blob.put(tab.data(), tab.size());
    o.off_vals = 0;
    if (s.maptype == 1 || s.maptype == 2) {
        const float mindel = float32_unpack(s.q_min), delta = float32_unpack(s.q_delta);
        const long qv = (long)s.quant.size();
        std::vector<float> vals((size_t)s.entries * s.dim, 0.f);
        for (int j = 0; j < s.entries; j++) {
            if (s.len[j] <= 0) continue;
            float last = 0.f;
            long indexdiv = 1;
            for (int k = 0; k < s.dim; k++) {
                const long index = s.maptype == 1 ? (j / indexdiv) % qv : (long)j * s.dim + k;
                float val = (float)s.quant[index];
                val = (float)(fabs(val) * delta + mindel + last);   // double arithmetic, as fabs() promotes in C
                if (s.q_seq) last = val;
                vals[(size_t)j * s.dim + k] = val;
                if (s.maptype == 1) indexdiv *= qv;
            }
        }
        o.off_vals = blob.put(vals.data(), vals.size());
    }
    return 0;
}

int unpack_floor1(vbmd_bits &b, vbmd_floor &f, int books)
{
    int count = 0, maxclass = -1;
    f.partitions = (int)vbmd_read(b, 5);
    if (f.partitions < 0) return -1;
    for (int j = 0; j < f.partitions; j++) {
        f.partclass[j] = (int)vbmd_read(b, 4);
        if (f.partclass[j] < 0) return -1;
        maxclass = std::max(maxclass, f.partclass[j]);
    }
    for (int j = 0; j < maxclass + 1; j++) {
        f.class_dim[j] = (int)vbmd_read(b, 3) + 1;
        f.class_subs[j] = (int)vbmd_read(b, 2);
        if (f.class_subs[j] < 0) return -1;
        f.class_book[j] = f.class_subs[j] ? (int)vbmd_read(b, 8) : 0;
        if (f.class_book[j] < 0 || f.class_book[j] >= books) return -1;
        for (int k = 0; k < (1 << f.class_subs[j]); k++) {
            f.subbook[j][k] = (int)vbmd_read(b, 8) - 1;
            if (f.subbook[j][k] < -1 || f.subbook[j][k] >= books) return -1;
        }
    }
    f.mult = (int)vbmd_read(b, 2) + 1;
    const int rangebits = (int)vbmd_read(b, 4);
    if (rangebits < 0) return -1;
    for (int j = 0, k = 0; j < f.partitions; j++) {
        count += f.class_dim[f.partclass[j]];
        if (count > VBMD_POSTS - 2) return -1;
        for (; k < count; k++) {
            const int t = f.postlist[k + 2] = (int)vbmd_read(b, rangebits);
            if (t < 0 || t >= (1 << rangebits)) return -1;
        }
    }
    f.postlist[0] = 0;
    f.postlist[1] = 1 << rangebits;
    f.posts = count + 2;
    std::vector<int> idx(f.posts);
    for (int j = 0; j < f.posts; j++) idx[j] = j;
    std::sort(idx.begin(), idx.end(), [&](int a, int c) { return f.postlist[a] < f.postlist[c]; });
    for (int j = 1; j < f.posts; j++)
        if (f.postlist[idx[j - 1]] == f.postlist[idx[j]]) return -1;     // zero-length segments
    for (int j = 0; j < f.posts; j++) f.fwd[j] = idx[j];
    static const int qq[4] = {256, 128, 86, 64};
    f.quant_q = qq[f.mult - 1];
    f.qbits = vbmd_ilog((unsigned)(f.quant_q - 1));
    for (int i = 0; i < f.posts - 2; i++) {
        int lo = 0, hi = 1, lx = 0, hx = f.postlist[1];
        const int cx = f.postlist[i + 2];
        for (int j = 0; j < i + 2; j++) {
            const int x = f.postlist[j];
            if (x > lx && x < cx) { lo = j; lx = x; }
            if (x < hx && x > cx) { hi = j; hx = x; }
        }
        f.lo[i] = lo;
        f.hi[i] = hi;
    }
    return 0;
}

int unpack_residue(vbmd_bits &b, vbmd_residue &r, const std::vector<Book> &books)
{
    int acc = 0;
    r.begin = (int)vbmd_read(b, 24);
    r.end = (int)vbmd_read(b, 24);
    r.grouping = (int)vbmd_read(b, 24) + 1;
    r.partitions = (int)vbmd_read(b, 6) + 1;
    r.groupbook = (int)vbmd_read(b, 8);
    if (r.groupbook < 0) return -1;
    for (int j = 0; j < r.partitions; j++) {
        int cascade = (int)vbmd_read(b, 3);
        const int cflag = (int)vbmd_read(b, 1);
        if (cflag < 0) return -1;
        if (cflag) {
            const int c = (int)vbmd_read(b, 5);
            if (c < 0) return -1;
            cascade |= c << 3;
        }
        r.secondstages[j] = cascade;
        acc += __builtin_popcount((unsigned)cascade);
    }
    std::vector<int> booklist(acc);
    for (int j = 0; j < acc; j++) {
        booklist[j] = (int)vbmd_read(b, 8);
        if (booklist[j] < 0) return -1;
    }
    if (r.groupbook >= (int)books.size()) return -1;
    for (int j = 0; j < acc; j++)
        if (booklist[j] >= (int)books.size() || books[booklist[j]].maptype == 0) return -1;
    // a stage book of dimension 0 would never advance the residue decode (the reference divides by it in
    // vorbis_book_decodevs_add and spins in decodev_add): rejected here, it cannot come from a working encoder
    for (int j = 0; j < acc; j++)
        if (books[booklist[j]].dim < 1) return -1;
    const int entries = books[r.groupbook].entries;
    int dim = books[r.groupbook].dim, partvals = 1;
    if (dim < 1) return -1;
    while (dim > 0) {
        partvals *= r.partitions;
        if (partvals > entries) return -1;
        dim--;
    }
    r.partvals = partvals;
    // res0_look
    r.stages = 0;
    for (int j = 0, k = 0; j < r.partitions; j++) {
        const int stages = vbmd_ilog((unsigned)r.secondstages[j]);
        r.stages = std::max(r.stages, stages);
        for (int s = 0; s < 8; s++) r.books[j][s] = -1;
        for (int s = 0; s < stages; s++)
            if (r.secondstages[j] & (1 << s)) r.books[j][s] = booklist[k++];
    }
    return 0;
}

int unpack_mapping(vbmd_bits &b, vbmd_mapping &m, int channels, int floors, int residues)
{
    int v = (int)vbmd_read(b, 1);
    if (v < 0) return -1;
    m.submaps = v ? (int)vbmd_read(b, 4) + 1 : 1;
    if (m.submaps <= 0) return -1;
    v = (int)vbmd_read(b, 1);
    if (v < 0) return -1;
    m.steps = 0;
    if (v) {
        m.steps = (int)vbmd_read(b, 8) + 1;
        if (m.steps <= 0) return -1;
        const int bits = vbmd_ilog((unsigned)(channels - 1));
        for (int i = 0; i < m.steps; i++) {
            const int M = (int)vbmd_read(b, bits), A = (int)vbmd_read(b, bits);
            if (M < 0 || A < 0 || M == A || M >= channels || A >= channels) return -1;
            m.mag[i] = (unsigned char)M;
            m.ang[i] = (unsigned char)A;
        }
    }
    if (vbmd_read(b, 2) != 0) return -1;
    for (int i = 0; i < channels; i++) m.mux[i] = 0;
    if (m.submaps > 1)
        for (int i = 0; i < channels; i++) {
            const int x = (int)vbmd_read(b, 4);
            if (x >= m.submaps || x < 0) return -1;
            m.mux[i] = (unsigned char)x;
        }
    for (int i = 0; i < m.submaps; i++) {
        vbmd_read(b, 8);
        const int fl = (int)vbmd_read(b, 8), rs = (int)vbmd_read(b, 8);
        if (fl >= floors || fl < 0 || rs >= residues || rs < 0) return -1;
        m.floorsub[i] = (unsigned char)fl;
        m.ressub[i] = (unsigned char)rs;
    }
    return 0;
}

bool header_sig(vbmd_bits &b, int &type)
{
    type = (int)vbmd_read(b, 8);
    char buf[6] = {};
    for (int i = 0; i < 6; i++) buf[i] = (char)vbmd_read(b, 8);
    return memcmp(buf, "vorbis", 6) == 0;
}

std::string lib_data_dir()
{
    if (const char *env = getenv("VORBIS_MI355X_DATA")) return env;
    Dl_info di;
    if (dladdr((const void *)&vbm_decode_setup_create, &di) && di.dli_fname) {
        std::string p = di.dli_fname;
        const size_t at = p.rfind('/');
        return (at == std::string::npos ? std::string(".") : p.substr(0, at)) + "/data";
    }
    return "data";
}

}  // namespace

// ---- floor line on the host: floor1_inverse2's render_line (lib/floor1.c:368), indices instead of products -----------
void vbmd_host_floor_index(const vbmd_setup &s, const vbmd_floor &f, const int *fit, int n, int *out)
{
    int hx = 0, lx = 0;
    int ly = fit[0] * f.mult;
    ly = ly < 0 ? 0 : ly > 255 ? 255 : ly;
    (void)s;
    for (int j = 1; j < f.posts; j++) {
        const int current = f.fwd[j];
        int hy = fit[current] & 0x7fff;
        if (hy != fit[current]) continue;
        hx = f.postlist[current];
        hy *= f.mult;
        hy = hy < 0 ? 0 : hy > 255 ? 255 : hy;
        // render_line(n, lx, hx, ly, hy, out)
        const int dy = hy - ly, adx = hx - lx;
        int ady = dy < 0 ? -dy : dy;
        const int base = dy / adx, sy = dy < 0 ? base - 1 : base + 1;
        int x = lx, y = ly, err = 0;
        ady -= (base < 0 ? -base : base) * adx;
        const int nn = n > hx ? hx : n;
        if (x < nn) out[x] = y;
        while (++x < nn) {
            err += ady;
            if (err >= adx) { err -= adx; y += sy; }
            else y += base;
            out[x] = y;
        }
        lx = hx;
        ly = hy;
    }
    for (int j = hx; j < n; j++) out[j] = ly;
}

int vbmd_setup_parse(vbm_decode_setup *ds, const uint8_t *headers, const long *lens)
{
    if (!ds || !headers || !lens) return VBM_EINVAL;
    for (int i = 0; i < 3; i++)
        if (lens[i] < 0) return VBM_EINVAL;
    const uint8_t *pk[3] = {headers, headers + lens[0], headers + lens[0] + lens[1]};
    vbmd_setup &s = ds->s;
    memset(&s, 0, sizeof(s));
    // vorbis_synthesis_headerin x3, in order: identification (b_o_s), comment, setup
    for (int h = 0; h < 3; h++) {
        vbmd_bits b = {pk[h], lens[h], 0};
        int type;
        if (!header_sig(b, type)) return VBM_ENOTVORBIS;
        if (type != 2 * h + 1) return VBM_EBADHEADER;      // out of order, or not a header type
        if (h == 0) {
            if (vbmd_read(b, 32) != 0) return VBM_EVERSION;
            s.channels = (int)vbmd_read(b, 8);
            s.rate = (int)vbmd_read(b, 32);
            for (int i = 0; i < 3; i++) vbmd_read(b, 32);
            const int b0 = (int)vbmd_read(b, 4), b1 = (int)vbmd_read(b, 4);
            s.blocksizes[0] = b0 < 0 ? 0 : 1 << b0;
            s.blocksizes[1] = b1 < 0 ? 0 : 1 << b1;
            if (s.rate < 1 || s.channels < 1 || s.blocksizes[0] < 64 || s.blocksizes[1] < s.blocksizes[0] ||
                s.blocksizes[1] > 8192)
                return VBM_EBADHEADER;
            if (vbmd_read(b, 1) != 1) return VBM_EBADHEADER;
        } else if (h == 1) {
            const long vlen = vbmd_read(b, 32);
            if (vlen < 0 || vlen > b.bytes - 8) return VBM_EBADHEADER;
            for (long i = 0; i < vlen; i++) vbmd_read(b, 8);
            const long nc = vbmd_read(b, 32);
            if (nc < 0 || nc > (b.bytes - (b.pos + 7) / 8) >> 2) return VBM_EBADHEADER;
            for (long i = 0; i < nc; i++) {
                const long l = vbmd_read(b, 32);
                if (l < 0 || l > b.bytes - (b.pos + 7) / 8) return VBM_EBADHEADER;
                for (long j = 0; j < l; j++) vbmd_read(b, 8);
            }
            if (vbmd_read(b, 1) != 1) return VBM_EBADHEADER;
        } else {
            s.books = (int)vbmd_read(b, 8) + 1;
            if (s.books <= 0) return VBM_EBADHEADER;
            std::vector<Book> books(s.books);
            for (int i = 0; i < s.books; i++)
                if (unpack_book(b, books[i])) return VBM_EBADHEADER;
            const int times = (int)vbmd_read(b, 6) + 1;
            if (times <= 0) return VBM_EBADHEADER;
            for (int i = 0; i < times; i++)
                if (vbmd_read(b, 16) != 0) return VBM_EBADHEADER;
            s.floors = (int)vbmd_read(b, 6) + 1;
            if (s.floors <= 0) return VBM_EBADHEADER;
            for (int i = 0; i < s.floors; i++) {
                const int type = (int)vbmd_read(b, 16);
                if (type < 0 || type >= 2) return VBM_EBADHEADER;
                if (type == 0) { g_vbm_err = "floor type 0 is not supported by the decoder"; return VBM_EIMPL; }
                if (unpack_floor1(b, s.floor[i], s.books)) return VBM_EBADHEADER;
            }
            s.residues = (int)vbmd_read(b, 6) + 1;
            if (s.residues <= 0) return VBM_EBADHEADER;
            for (int i = 0; i < s.residues; i++) {
                s.res[i].type = (int)vbmd_read(b, 16);
                if (s.res[i].type < 0 || s.res[i].type >= 3) return VBM_EBADHEADER;
                if (unpack_residue(b, s.res[i], books)) return VBM_EBADHEADER;
            }
            s.maps = (int)vbmd_read(b, 6) + 1;
            if (s.maps <= 0) return VBM_EBADHEADER;
            for (int i = 0; i < s.maps; i++) {
                if (vbmd_read(b, 16) != 0) return VBM_EBADHEADER;
                if (s.channels > VBMD_MAXCH) break;             // reported below as VBM_EIMPL
                if (unpack_mapping(b, s.map[i], s.channels, s.floors, s.residues)) return VBM_EBADHEADER;
            }
            if (s.channels > VBMD_MAXCH) { g_vbm_err = "more than 8 channels"; return VBM_EIMPL; }
            s.modes = (int)vbmd_read(b, 6) + 1;
            if (s.modes <= 0) return VBM_EBADHEADER;
            for (int i = 0; i < s.modes; i++) {
                s.mode_blockflag[i] = (int)vbmd_read(b, 1);
                const long wt = vbmd_read(b, 16), tt = vbmd_read(b, 16);
                s.mode_mapping[i] = (int)vbmd_read(b, 8);
                if (wt >= 1 || tt >= 1 || s.mode_mapping[i] >= s.maps || s.mode_mapping[i] < 0) return VBM_EBADHEADER;
            }
            if (vbmd_read(b, 1) != 1) return VBM_EBADHEADER;
            s.modebits = vbmd_ilog((unsigned)(s.modes - 1));
            // vorbis_book_init_decode (vorbis_synthesis_init: a book that does not form a complete tree fails there)
            Blob blob;
            for (int i = 0; i < s.books; i++)
                if (build_book(books[i], s.book[i], blob)) return VBM_EBADHEADER;
            ds->blob = std::move(blob.d);
            s.blob_bytes = (uint32_t)ds->blob.size();
        }
    }
    if (s.blocksizes[0] < 256 || s.blocksizes[1] > 4096) {
        g_vbm_err = "block sizes outside 256..4096 are not supported by the decoder";
        return VBM_EIMPL;
    }
    // partition-class scratch of one packet (largest block)
    long maxc = 1;
    const int n = s.blocksizes[1] / 2;
    for (int i = 0; i < s.residues; i++) {
        const vbmd_residue &r = s.res[i];
        const long max = r.type == 2 ? (long)n * s.channels : n;
        const long len = std::min<long>(r.end, max) - r.begin;
        if (len > 0) maxc = std::max(maxc, (len / r.grouping) * (r.type == 2 ? 1 : s.channels));
    }
    s.max_classes = (int)((maxc + 15) & ~15L);
    // the tables the device path needs: windows of both block sizes and of half each, FLOOR1_fromdB_LOOKUP (common.vpk)
    const int sizes[4] = {s.blocksizes[0], s.blocksizes[1], s.blocksizes[0] / 2, s.blocksizes[1] / 2};
    std::vector<float> *win[4] = {&ds->win[0], &ds->win[1], &ds->hwin[0], &ds->hwin[1]};
    return vbmd_common_tables(&ds->fromdB, 4, sizes, win);
}

int vbmd_common_tables(std::vector<float> *fromdB, int n, const int *sizes, std::vector<float> *const *win)
{
    const std::string path = lib_data_dir() + "/common.vpk";
    vpk_file f;
    if (vpk_open(&f, path.c_str())) { g_vbm_err = "cannot open " + path; return VBM_EFAULT; }
    size_t cnt = 0;
    const float *db = (const float *)vpk_get(&f, "FLOOR1_fromdB_LOOKUP", VPK_F32, &cnt);
    bool ok = db && cnt == 256;
    if (ok) fromdB->assign(db, db + 256);
    for (int i = 0; i < n && ok; i++) {
        const std::string name = "window/" + std::to_string(sizes[i]);
        const float *w = (const float *)vpk_get(&f, name.c_str(), VPK_F32, &cnt);
        ok = w && (int)cnt == sizes[i] / 2;
        if (ok) win[i]->assign(w, w + cnt);
    }
    vpk_close(&f);
    if (!ok) { g_vbm_err = "common.vpk lacks a decode table"; return VBM_EFAULT; }
    return VBM_OK;
}

extern "C" int vbm_decode_setup_create(vbm_decode_setup **out, const uint8_t *headers, const long *lens)
{
    if (!out) return VBM_EINVAL;
    *out = nullptr;
    vbm_decode_setup *ds = new vbm_decode_setup();
    const int rc = vbmd_setup_parse(ds, headers, lens);
    if (rc) { delete ds; return rc; }
    *out = ds;
    return VBM_OK;
}

extern "C" void vbm_decode_setup_destroy(vbm_decode_setup *ds) { delete ds; }

extern "C" int vbm_decode_setup_info(const vbm_decode_setup *ds, int *channels, long *rate, int *blocksizes, int *modes)
{
    if (!ds) return VBM_EINVAL;
    if (channels) *channels = ds->s.channels;
    if (rate) *rate = ds->s.rate;
    if (blocksizes) { blocksizes[0] = ds->s.blocksizes[0]; blocksizes[1] = ds->s.blocksizes[1]; }
    if (modes) *modes = ds->s.modes;
    return VBM_OK;
}

extern "C" int vbm_decode_setup_counts(const vbm_decode_setup *ds, int *counts)
{
    if (!ds || !counts) return VBM_EINVAL;
    counts[0] = ds->s.books;
    counts[1] = ds->s.floors;
    counts[2] = ds->s.residues;
    counts[3] = ds->s.maps;
    return VBM_OK;
}

void vbmd_index_stream(const vbmd_setup &s, int halfrate, long long n, const uint8_t *data, const long long *offsets,
                       long long data_bytes, const long long *granulepos, const uint8_t *eos, int *status, int *begin,
                       int *end, long long *out_start, long long *total)
{
    int lW = -1;
    long long sc = -1, gp = -1, at = 0;
    for (long long k = 0; k < n; k++) {
        long long b = offsets[k], e = offsets[k + 1];
        b = b < 0 ? 0 : b > data_bytes ? data_bytes : b;
        e = e < b ? b : e > data_bytes ? data_bytes : e;
        vbmd_bits bits = {data + b, (long)(e - b), 0};
        int mode, W, plW, nW;
        status[k] = vbmd_head(s, bits, mode, W, plW, nW);
        long pb = 0, pe = 0;
        if (status[k] == 0) {
            const long long vgp = granulepos ? granulepos[k] : -1;
            const int eof = eos ? eos[k] : 0;
            if (halfrate) vbmd_blockin<1>(s.blocksizes, lW, W, vgp, eof, sc, gp, pb, pe);
            else vbmd_blockin<0>(s.blocksizes, lW, W, vgp, eof, sc, gp, pb, pe);
            lW = W;
        }
        if (begin) begin[k] = (int)pb;
        if (end) end[k] = (int)pe;
        out_start[k] = at;
        at += pe - pb;
    }
    *total = at;
}

extern "C" int vbm_decode_index(const vbm_decode_setup *ds, long long npackets, const uint8_t *data,
                                const long long *offsets, long long data_bytes, const long long *granulepos,
                                const uint8_t *eos, int *status, int *samples, long long *out_start, long long *total)
{
    return vbm_decode_index_halfrate(ds, 0, npackets, data, offsets, data_bytes, granulepos, eos, status, samples,
                                     out_start, total);
}

extern "C" int vbm_decode_index_halfrate(const vbm_decode_setup *ds, int halfrate, long long npackets,
                                         const uint8_t *data, const long long *offsets, long long data_bytes,
                                         const long long *granulepos, const uint8_t *eos, int *status, int *samples,
                                         long long *out_start, long long *total)
{
    if (halfrate != 0 && halfrate != 1) { g_vbm_err = "halfrate must be 0 or 1"; return VBM_EINVAL; }
    if (!ds || npackets < 0 || data_bytes < 0 || (data_bytes > 0 && !data) || !offsets || !total ||
        (npackets > 0 && (!status || !samples || !out_start)))
        return VBM_EINVAL;
    std::vector<int> b((size_t)npackets), e((size_t)npackets);
    vbmd_index_stream(ds->s, halfrate, npackets, data, offsets, data_bytes, granulepos, eos, status, b.data(), e.data(),
                      out_start, total);
    for (long long k = 0; k < npackets; k++) samples[k] = e[k] - b[k];
    return VBM_OK;
}

extern "C" int vbm_host_unpack_packet(const vbm_decode_setup *ds, const uint8_t *packet, long bytes, int *info,
                                      int *floor_index, float *residue, int *floor_used)
{
    if (!ds || (!packet && bytes > 0) || bytes < 0 || !info) return VBM_EINVAL;
    const vbmd_setup &s = ds->s;
    const long half = s.blocksizes[1] / 2;
    std::vector<int> fit((size_t)s.channels * VBMD_POSTS, 0), flags(s.channels, 0);
    std::vector<float> res((size_t)s.channels * half, 0.f);
    std::vector<uint8_t> cls(s.max_classes, 0);
    const int rc = vbmd_unpack(s, ds->blob.data(), packet, bytes, info, fit.data(), flags.data(), res.data(), half,
                               cls.data());
    if (floor_index) {
        std::fill(floor_index, floor_index + s.channels * half, 0);
        if (rc == 0) {
            const vbmd_mapping &m = s.map[s.mode_mapping[info[0]]];
            const int n = s.blocksizes[info[1]] / 2;
            for (int c = 0; c < s.channels; c++)
                if (flags[c] & 1)
                    vbmd_host_floor_index(s, s.floor[m.floorsub[m.mux[c]]], &fit[(size_t)c * VBMD_POSTS], n,
                                          floor_index + c * half);
        }
    }
    if (residue) memcpy(residue, res.data(), res.size() * sizeof(float));
    if (floor_used)
        for (int c = 0; c < s.channels; c++) floor_used[c] = (flags[c] >> 1) & 1;
    return rc;
}
