// jpegd_header.h — host-only parser of a JPEG image's header, SOI through SOS,
// into the decoder's tables and geometry (DESIGN.md "Motion-JPEG decoder",
// accepted streams). Plain C++: jpegd_api.hip and tools/jpegd_host_check.cc
// share it.
#pragma once
#include <stddef.h>
#include <string.h>

#include "jpeg_std_tables.h"
#include "jpegd_core.h"

namespace dvc {

enum { kJpegdOk = 0, kJpegdInvalid = -1, kJpegdUnsupported = -5 };   // DVC_OK, DVC_E_INVALID, DVC_E_UNSUPPORTED

// Natural index of zigzag position k.
static const uint8_t kJpegdNat[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                      41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                      30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct JpegdHeader {
    JpegdGeom g;
    JpegdTables t;
    size_t length;   // bytes up to and including the SOS header: the entropy data follows
};

// Parses d[0, n). On success fills *out and returns kJpegdOk; otherwise returns
// kJpegdInvalid (not a header, cut short, inconsistent) or kJpegdUnsupported (a
// JPEG this decoder does not take) with *why naming the reason and *out
// unspecified. Nothing outside d[0, n) is read. `camera` (DVC_FLAG_JPEGD_CAMERA)
// widens the set: 4:2:2 (2x1) and 4:4:4 luma factors, and a scan whose Huffman
// tables no DHT defined means the Annex K ones; it refuses RGB-coded streams by
// libjpeg's rule (no JFIF APP0 and an Adobe APP14 with transform 0, or neither
// and the component ids 'R', 'G', 'B').
inline int jpegd_parse_header(const uint8_t* d, size_t n, JpegdHeader* out, const char** why, bool camera = false)
{
    const char* dummy;
    if (!why) why = &dummy;
    *why = "";
    if (n < 4 || d[0] != 0xff || d[1] != 0xd8) return *why = "no SOI marker", kJpegdInvalid;
    uint8_t qt[4][64];
    bool have_q[4] = {false, false, false, false}, have_h[2][2] = {{false, false}, {false, false}};
    bool have_sof = false;
    JpegdHeader& o = *out;
    memset(&o, 0, sizeof(o));
    memcpy(o.t.nat, kJpegdNat, 64);
    int nc = 0, dri = 0, cid[3] = {0, 0, 0}, cq[3] = {0, 0, 0}, hs = 1, vs = 1;
    bool jfif = false, adobe = false;
    int adobe_transform = 0;
    size_t p = 2;
    for (;;) {
        if (p + 4 > n) return *why = "header cut short", kJpegdInvalid;
        if (d[p] != 0xff) return *why = "marker expected", kJpegdInvalid;
        const int m = d[p + 1];
        if (m == 0xff) {   // fill byte
            ++p;
            continue;
        }
        const size_t ln = (size_t)d[p + 2] << 8 | d[p + 3];
        if (ln < 2 || p + 2 + ln > n) return *why = "header cut short", kJpegdInvalid;
        const uint8_t* b = d + p + 4;
        const size_t bl = ln - 2;
        p += 2 + ln;
        if (m == 0xe0 && bl >= 5 && memcmp(b, "JFIF", 5) == 0) jfif = true;
        if (m == 0xee && bl >= 12 && memcmp(b, "Adobe", 5) == 0) {
            adobe = true;
            adobe_transform = b[11];
        }
        if ((m >= 0xe0 && m <= 0xef) || m == 0xfe) continue;   // APPn, COM
        if (m == 0xdb) {
            size_t i = 0;
            while (i < bl) {
                if (b[i] >> 4) return *why = "16-bit quantiser table", kJpegdUnsupported;
                const int id = b[i] & 15;
                if (id > 3 || i + 65 > bl) return *why = "bad DQT", kJpegdInvalid;
                memcpy(qt[id], b + i + 1, 64);
                have_q[id] = true;
                i += 65;
            }
        } else if (m == 0xc4) {
            size_t i = 0;
            while (i < bl) {
                if (i + 17 > bl) return *why = "bad DHT", kJpegdInvalid;
                const int cls = b[i] >> 4, id = b[i] & 15;
                int cnt = 0;
                for (int l = 0; l < 16; ++l) cnt += b[i + 1 + l];
                if (cls > 1 || cnt > 256 || i + 17 + cnt > bl) return *why = "bad DHT", kJpegdInvalid;
                if (id > 1) return *why = "more than two Huffman tables of a class", kJpegdUnsupported;
                JpegdHuff* h = cls ? &o.t.ac[id] : &o.t.dc[id];
                if (!jpegd_build_huff(b + i + 1, b + i + 17, cnt, h)) return *why = "bad DHT", kJpegdInvalid;
                have_h[cls][id] = true;
                i += 17 + (size_t)cnt;
            }
        } else if (m == 0xc0) {
            if (have_sof) return *why = "two frame headers", kJpegdInvalid;
            if (bl < 6) return *why = "bad SOF", kJpegdInvalid;
            if (b[0] != 8) return *why = "sample precision other than 8 bits", kJpegdUnsupported;
            o.g.H = b[1] << 8 | b[2];
            o.g.W = b[3] << 8 | b[4];
            nc = b[5];
            if (bl != 6 + 3 * (size_t)nc) return *why = "bad SOF", kJpegdInvalid;
            if (nc != 1 && nc != 3) return *why = "component count other than 1 or 3", kJpegdUnsupported;
            if (o.g.W < 1 || o.g.H < 1) return *why = "empty frame", kJpegdInvalid;
            for (int c = 0; c < nc; ++c) {
                cid[c] = b[6 + 3 * c];
                const int hv = b[7 + 3 * c];
                cq[c] = b[8 + 3 * c];
                if (cq[c] > 3) return *why = "bad SOF", kJpegdInvalid;
                // (a single component's factors do not matter: its scan is not interleaved)
                if (nc == 3 && hv != (c == 0 ? 0x22 : 0x11)) {
                    if (!camera) return *why = "sampling other than 4:2:0", kJpegdUnsupported;
                    if (c != 0 || (hv != 0x21 && hv != 0x11))
                        return *why = "sampling other than 4:2:0, 4:2:2 (2x1) and 4:4:4", kJpegdUnsupported;
                }
                if (nc == 3 && c == 0) {
                    hs = hv >> 4;
                    vs = hv & 15;
                }
            }
            have_sof = true;
        } else if (m == 0xc1 || m == 0xc2 || m == 0xc3 || (m >= 0xc5 && m <= 0xcf && m != 0xc8 && m != 0xcc)) {
            return *why = "not a baseline Huffman frame (SOF0)", kJpegdUnsupported;
        } else if (m == 0xcc) {
            return *why = "arithmetic coding", kJpegdUnsupported;
        } else if (m == 0xdd) {
            if (bl != 2) return *why = "bad DRI", kJpegdInvalid;
            dri = b[0] << 8 | b[1];
        } else if (m == 0xda) {
            if (!have_sof) return *why = "scan before the frame header", kJpegdInvalid;
            if (bl < 1 || bl != 4 + 2 * (size_t)b[0]) return *why = "bad SOS", kJpegdInvalid;
            if (b[0] != nc) return *why = "more than one scan", kJpegdUnsupported;
            for (int c = 0; c < nc; ++c) {
                if (b[1 + 2 * c] != cid[c]) return *why = "scan components out of order", kJpegdUnsupported;
                const int td = b[2 + 2 * c] >> 4, ta = b[2 + 2 * c] & 15;
                if (td > 1 || ta > 1) return *why = "more than two Huffman tables of a class", kJpegdUnsupported;
                if (!have_h[0][td] || !have_h[1][ta]) {
                    if (!camera) return *why = "scan names a missing Huffman table", kJpegdInvalid;
                    for (int cls = 0; cls < 2; ++cls) {   // the Annex K table of the slot
                        const int id = cls ? ta : td;
                        if (have_h[cls][id]) continue;
                        const JpegStdTable s = jpeg_std_table(cls, id);
                        if (!jpegd_build_huff(s.bits, s.vals, s.nvals, cls ? &o.t.ac[id] : &o.t.dc[id]))
                            return *why = "bad DHT", kJpegdInvalid;
                        have_h[cls][id] = true;
                    }
                }
                if (!have_q[cq[c]]) return *why = "frame names a missing quantiser table", kJpegdInvalid;
                o.t.dc_sel[c] = (uint8_t)td;
                o.t.ac_sel[c] = (uint8_t)ta;
                for (int k = 0; k < 64; ++k) o.t.q[c][kJpegdNat[k]] = qt[cq[c]][k];
            }
            if (b[1 + 2 * nc] != 0 || b[2 + 2 * nc] != 63 || b[3 + 2 * nc] != 0)
                return *why = "not a sequential scan", kJpegdUnsupported;
            if (camera && nc == 3 && !jfif &&
                (adobe ? adobe_transform == 0 : (cid[0] == 'R' && cid[1] == 'G' && cid[2] == 'B')))
                return *why = "RGB-coded components", kJpegdUnsupported;
            break;
        } else {
            return *why = "unexpected marker", kJpegdInvalid;
        }
    }
    JpegdGeom& g = o.g;
    g.gray = nc == 1;
    g.hs = g.gray ? 1 : hs;
    g.vs = g.gray ? 1 : vs;
    const int mw = 8 * g.hs, mh = 8 * g.vs;
    g.mcus_x = (g.W + mw - 1) / mw;
    g.mcus_y = (g.H + mh - 1) / mh;
    g.mcus = g.mcus_x * g.mcus_y;
    g.ri = dri ? (dri < g.mcus ? dri : g.mcus) : g.mcus;
    g.nseg = (g.mcus + g.ri - 1) / g.ri;
    g.bpm = g.gray ? 1 : g.hs * g.vs + 2;
    g.yw = g.mcus_x * mw;
    g.yh = g.mcus_y * mh;
    g.cw = g.gray ? 0 : g.mcus_x * 8;
    g.ch = g.gray ? 0 : g.mcus_y * 8;
    o.length = p;
    return kJpegdOk;
}

}  // namespace dvc
