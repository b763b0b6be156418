// jpezy_exif.h -- the EXIF Orientation tag of a JPEG file and the geometry of the eight orientations (include/jpezy_hip_orientation.h).
// Plain C++, no HIP, no dependency on the rest of the library: a stand-alone program can include it (the parser reads untrusted offsets
// and is run under a sanitizer that way).  Every read goes through Bytes::u8, which knows the end of what may be read.
#pragma once
#include <cstddef>
#include <cstdint>

namespace jpezy_exif {

// a span that answers -1 outside itself: no pointer is formed past the end
struct Bytes {
    const uint8_t* p;
    size_t n;
    int u8(size_t at) const { return at < n ? (int)p[at] : -1; }
    // 16 / 32 bits at `at` in the TIFF header's byte order; -1 when any byte lies outside
    long long u16(size_t at, bool big) const
    {
        if (at >= n || n - at < 2) return -1;
        return big ? ((long long)p[at] << 8) | p[at + 1] : ((long long)p[at + 1] << 8) | p[at];
    }
    long long u32(size_t at, bool big) const
    {
        if (at >= n || n - at < 4) return -1;
        return big ? ((long long)p[at] << 24) | ((long long)p[at + 1] << 16) | ((long long)p[at + 2] << 8) | p[at + 3]
                   : ((long long)p[at + 3] << 24) | ((long long)p[at + 2] << 16) | ((long long)p[at + 1] << 8) | p[at];
    }
};

// the tag in one TIFF structure (what follows "Exif\0\0" in the APP1 payload): IFD0 only, tag 0x0112, SHORT or LONG, count 1.
// 0: not there, malformed, or a value outside 1..8
inline int tiff_orientation(const Bytes& t)
{
    bool big;
    if (t.u8(0) == 'I' && t.u8(1) == 'I') big = false;
    else if (t.u8(0) == 'M' && t.u8(1) == 'M') big = true;
    else return 0;
    if (t.u16(2, big) != 42) return 0;
    const long long ifd = t.u32(4, big);
    if (ifd < 8) return 0;                                    // (inside the header, or -1)
    const long long count = t.u16((size_t)ifd, big);
    if (count < 0) return 0;                                  // the IFD offset lies past the segment
    // every entry of the directory must lie in the segment, looked at or not
    if ((unsigned long long)ifd + 2 + (unsigned long long)count * 12 > t.n) return 0;
    for (long long k = 0; k < count; ++k) {
        const size_t e = (size_t)ifd + 2 + (size_t)k * 12;
        if (t.u16(e, big) != 0x0112) continue;
        const long long type = t.u16(e + 2, big), n = t.u32(e + 4, big);
        if (n != 1) return 0;
        long long v;
        if (type == 3) v = t.u16(e + 8, big);                 // SHORT: left-justified in the value field
        else if (type == 4) v = t.u32(e + 8, big);            // LONG
        else return 0;
        return v >= 1 && v <= 8 ? (int)v : 0;
    }
    return 0;
}

// The file's orientation: the first APP1 in front of SOS whose payload starts with "Exif\0\0" decides.  1 when anything is missing or
// wrong.  Reads data[0, len) only.
inline int jpeg_orientation(const uint8_t* data, size_t len)
{
    if (!data || len < 4) return 1;
    const Bytes f = { data, len };
    if (f.u8(0) != 0xFF || f.u8(1) != 0xD8) return 1;
    size_t at = 2;
    for (;;) {
        if (f.u8(at) != 0xFF) return 1;
        int mk = f.u8(at + 1);
        while (mk == 0xFF) { ++at; mk = f.u8(at + 1); }       // fill bytes in front of a marker
        if (mk < 0 || mk == 0xDA || mk == 0xD9) return 1;     // the end, the scan, the end of the image
        at += 2;
        if (mk == 0x01 || (mk >= 0xD0 && mk <= 0xD7)) continue;   // markers without a segment
        const long long seg = f.u16(at, true);
        if (seg < 2 || (unsigned long long)seg > len - at) return 1;   // at <= len here: u16 answered
        if (mk == 0xE1 && seg >= 8) {
            const uint8_t* s = data + at + 2;
            if (s[0] == 'E' && s[1] == 'x' && s[2] == 'i' && s[3] == 'f' && s[4] == 0 && s[5] == 0) {
                const int o = tiff_orientation({ s + 6, (size_t)seg - 8 });
                return o ? o : 1;
            }
        }
        at += (size_t)seg;
    }
}

// ---- geometry: O = orient(P, o), P of W x H pixels (include/jpezy_hip_orientation.h's table) ----
// O[Y][X] = P[sy][sx] with (a, b) = transposed ? (Y, X) : (X, Y), sx = mirror_x ? W - 1 - a : a, sy = mirror_y ? H - 1 - b : b
constexpr int kTranspose = 1, kMirrorX = 2, kMirrorY = 4;
// o in 1..8
inline int orient_bits(int o)
{
    constexpr int bits[8] = { 0, kMirrorX, kMirrorX | kMirrorY, kMirrorY, kTranspose, kTranspose | kMirrorY, kTranspose | kMirrorX | kMirrorY,
                              kTranspose | kMirrorX };
    return bits[o - 1];
}

struct Rect { int x, y, w, h; };
// the source-side rectangle of the oriented window r (inside the oriented picture; o in 1..8)
inline Rect orient_rect(int o, int W, int H, const Rect& r)
{
    const int b = orient_bits(o);
    // the window's extent along the axis that becomes the source's x, and along the one that becomes its y
    const int a0 = (b & kTranspose) ? r.y : r.x, an = (b & kTranspose) ? r.h : r.w;
    const int b0 = (b & kTranspose) ? r.x : r.y, bn = (b & kTranspose) ? r.w : r.h;
    return { (b & kMirrorX) ? W - a0 - an : a0, (b & kMirrorY) ? H - b0 - bn : b0, an, bn };
}

}  // namespace jpezy_exif
