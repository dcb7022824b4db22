// The bytes of a detection CSV line, written once for the host compiler and for hipcc (csrc/csv.hip): plain C++, no library
// call, no private array -- every digit is stored straight to the caller's buffer (a per-lane slot in LDS on the device).
//
//   csvf::f32_decimal  a finite non-zero float32, widened exactly to double, -> the shortest decimal digit string that reads
//                      back as THAT DOUBLE (the closest one where several have that length), as an integer `digits` of n
//                      digits and the position of the decimal point `decpt` (value = 0.d1 d2 .. dn * 10^decpt): what
//                      Python's repr(float(np.float32)) prints.  The rounding interval is the double's, 2^-53 relative -- this
//                      is why float32(0.1) has seventeen digits -- and below a power of two it is half as wide as above it
//                      (`mm_shift`).  The routine is Ryu (Adams, PLDI 2018) with the 128-bit powers of five of csv_pow5.hpp
//                      (tools/gen_csv_pow5.py), cut to the exponents a widened float32 has.
//   csvf::f32_len / f32_put   repr's text: fixed notation for -4 < decpt <= 16 with ".0" behind an integer, else d.ddde-05 /
//                      1e+16 with at least two exponent digits; "-0.0", "nan" (any sign, any payload), "inf", "-inf".
//   csvf::int_len / int_put   str(int).
//   csvf::line_len / line_put  "frame,class,id,x,y,z\n", at most CSVF_LINE_MAX bytes.
// len and put share one decomposition, so a length pass and a write pass cannot disagree.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CSVF_FN __host__ __device__ inline
#define CSVF_TABLE __device__ const
#else
#define CSVF_FN inline
#define CSVF_TABLE static const
#endif
#if defined(__HIPCC__) && !defined(__HIP_DEVICE_COMPILE__)
// the host half of a hipcc translation unit never formats: the tables live on the device only
#define CSVF_NO_TABLES 1
#endif

#include "csv_pow5.hpp"

#define CSVF_LINE_MAX 110      // 10 (frame) + 11 (class) + 10 (id) + 3 * 23 (floats) + 5 commas + newline = 106

namespace csvf {

static_assert(CSVF_POW5_BITS == 125, "mul_shift's shifts are those of 125-bit powers");
static_assert(CSVF_POW5_INV_N >= 22 && CSVF_POW5_N >= 64, "a widened float32 needs 10^-21 .. and 5^63");

struct Decimal {
    uint64_t digits;      // n decimal digits, the first non-zero
    int n;
    int decpt;
};

CSVF_FN uint64_t mul_hi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// (m * (hi:lo)) >> j for 64 < j < 128; the product has at most 64 + 125 bits and the result fits 64
CSVF_FN uint64_t mul_shift(uint64_t m, uint64_t lo, uint64_t hi, int j) {
    const uint64_t b0_hi = mul_hi64(m, lo);
    const uint64_t b2_lo = m * hi, b2_hi = mul_hi64(m, hi);
    const uint64_t mid = b0_hi + b2_lo;                         // bits 64 .. 127 of the product
    const uint64_t top = b2_hi + (mid < b0_hi ? 1u : 0u);       // bits 128 ..
    const int s = j - 64;
    return (mid >> s) | (top << (64 - s));
}

CSVF_FN int pow5bits(int e) { return (int)(((uint32_t)e * 1217359u) >> 19) + 1; }
CSVF_FN int log10_pow2(int e) { return (int)(((uint32_t)e * 78913u) >> 18); }
CSVF_FN int log10_pow5(int e) { return (int)(((uint32_t)e * 732923u) >> 20); }

CSVF_FN bool multiple_of_pow5(uint64_t v, int p) {
    int c = 0;
    while (v != 0 && v % 5 == 0) {
        v /= 5;
        ++c;
    }
    return c >= p;
}

CSVF_FN int decimal_digits(uint64_t v) {                        // 1 .. 17
    int n = 1;
    for (uint64_t p = 10; n < 20 && v >= p; p *= 10) ++n;
    return n;
}

// bits: a float32 that is finite and not zero (the sign is not read)
CSVF_FN Decimal f32_decimal(uint32_t bits) {
    const uint32_t mant = bits & 0x7fffffu, fexp = (bits >> 23) & 0xffu;
    // the double m2 * 2^(e2 + 2), m2 with 53 bits
    uint64_t m2;
    int e2;
    bool mm_shift;                                              // false: m2 is 2^52, the lower neighbour is half as far
    if (fexp != 0) {
        m2 = (uint64_t)(0x800000u | mant) << 29;
        e2 = (int)fexp - 127 - 52 - 2;
        mm_shift = mant != 0;
    } else {
        int p = 22;
        while (!((mant >> p) & 1u)) --p;                        // (mant != 0)
        m2 = (uint64_t)mant << (52 - p);
        e2 = p - 149 - 52 - 2;
        mm_shift = (mant & (mant - 1u)) != 0;
    }
    const uint64_t mv = 4 * m2, mp = mv + 2, mm = mv - 1 - (mm_shift ? 1 : 0);
    // the low 29 bits of m2 are zero: it is even, and the bounds themselves read back as the double (round half to even)
    uint64_t vr, vp, vm;
    int e10;
    bool vm_tz = false, vr_tz = false;
#if defined(CSVF_NO_TABLES)
    vr = vp = vm = 0, e10 = 0, (void)mp, (void)mm, (void)e2;
#else
    if (e2 >= 0) {
        const int q = log10_pow2(e2) - (e2 > 3 ? 1 : 0);
        e10 = q;
        const int j = -e2 + q + CSVF_POW5_BITS + pow5bits(q) - 1;
        const uint64_t lo = CSVF_POW5_INV[q][0], hi = CSVF_POW5_INV[q][1];
        vr = mul_shift(mv, lo, hi, j), vp = mul_shift(mp, lo, hi, j), vm = mul_shift(mm, lo, hi, j);
        if (q <= 21) {
            if (mv % 5 == 0) vr_tz = multiple_of_pow5(mv, q);
            else vm_tz = multiple_of_pow5(mm, q);
        }
    } else {
        const int q = log10_pow5(-e2) - (-e2 > 1 ? 1 : 0);
        e10 = q + e2;
        const int i = -e2 - q;
        const int j = q - (pow5bits(i) - CSVF_POW5_BITS);
        const uint64_t lo = CSVF_POW5[i][0], hi = CSVF_POW5[i][1];
        vr = mul_shift(mv, lo, hi, j), vp = mul_shift(mp, lo, hi, j), vm = mul_shift(mm, lo, hi, j);
        if (q <= 1) {
            vr_tz = true;
            vm_tz = mm_shift;                                   // mm = mv - 2 has its one trailing zero bit, mv - 1 none
        } else if (q < 63) {
            vr_tz = (mv & ((1ull << q) - 1)) == 0;
        }
    }
#endif
    int removed = 0;
    uint32_t last = 0;
    uint64_t out;
    if (vm_tz || vr_tz) {
        while (vp / 10 > vm / 10) {
            vm_tz &= vm % 10 == 0;
            vr_tz &= last == 0;
            last = (uint32_t)(vr % 10);
            vr /= 10, vp /= 10, vm /= 10;
            ++removed;
        }
        if (vm_tz) {
            while (vm % 10 == 0) {
                vr_tz &= last == 0;
                last = (uint32_t)(vr % 10);
                vr /= 10, vp /= 10, vm /= 10;
                ++removed;
            }
        }
        if (vr_tz && last == 5 && vr % 2 == 0) last = 4;        // exactly half way: to even
        out = vr + (((vr == vm && !vm_tz) || last >= 5) ? 1 : 0);
    } else {
        bool up = false;
        while (vp / 10 > vm / 10) {
            up = vr % 10 >= 5;
            vr /= 10, vp /= 10, vm /= 10;
            ++removed;
        }
        out = vr + ((vr == vm || up) ? 1 : 0);
    }
    Decimal d;
    d.digits = out;
    d.n = decimal_digits(out);
    d.decpt = e10 + removed + d.n;
    return d;
}

CSVF_FN int int_len(int64_t v) {
    uint64_t u = v < 0 ? (uint64_t)(-v) : (uint64_t)v;
    return decimal_digits(u) + (v < 0 ? 1 : 0);
}

// the n digits of u at p[0 .. n)
CSVF_FN void put_digits(char *p, uint64_t u, int n) {
    for (int k = n - 1; k >= 0; --k) {
        p[k] = (char)('0' + (int)(u % 10));
        u /= 10;
    }
}

CSVF_FN int int_put(char *p, int64_t v) {
    const uint64_t u = v < 0 ? (uint64_t)(-v) : (uint64_t)v;
    const int n = decimal_digits(u), neg = v < 0 ? 1 : 0;
    if (neg) p[0] = '-';
    put_digits(p + neg, u, n);
    return n + neg;
}

// repr(float(np.float32)) of the float32 `bits`.  PUT false: only the length (p is not touched).
template <bool PUT>
CSVF_FN int f32_text(char *p, uint32_t bits) {
    const uint32_t mag = bits & 0x7fffffffu;
    const int neg = (bits >> 31) ? 1 : 0;
    if (mag > 0x7f800000u) {
        if (PUT) p[0] = 'n', p[1] = 'a', p[2] = 'n';
        return 3;
    }
    if (PUT && neg) *p++ = '-';
    if (mag == 0x7f800000u) {
        if (PUT) p[0] = 'i', p[1] = 'n', p[2] = 'f';
        return neg + 3;
    }
    if (mag == 0) {
        if (PUT) p[0] = '0', p[1] = '.', p[2] = '0';
        return neg + 3;
    }
    const Decimal d = f32_decimal(bits);
    const int n = d.n, decpt = d.decpt;
    if (-4 < decpt && decpt <= 16) {
        if (decpt <= 0) {                                       // 0.000ddd
            if (PUT) {
                p[0] = '0', p[1] = '.';
                for (int k = 0; k < -decpt; ++k) p[2 + k] = '0';
                put_digits(p + 2 - decpt, d.digits, n);
            }
            return neg + 2 - decpt + n;
        }
        if (decpt >= n) {                                       // ddd000.0
            if (PUT) {
                put_digits(p, d.digits, n);
                for (int k = n; k < decpt; ++k) p[k] = '0';
                p[decpt] = '.', p[decpt + 1] = '0';
            }
            return neg + decpt + 2;
        }
        if (PUT) {                                              // dd.ddd: the digits, then the tail moved one place up
            put_digits(p, d.digits, n);
            for (int k = n; k > decpt; --k) p[k] = p[k - 1];
            p[decpt] = '.';
        }
        return neg + n + 1;
    }
    int e = decpt - 1;                                          // d.ddde-05
    const int frac = n > 1 ? n : 0;                             // '.' and n - 1 digits
    const int ea = e < 0 ? -e : e, en = ea >= 100 ? 3 : 2;
    if (PUT) {
        put_digits(p + (n > 1 ? 1 : 0), d.digits, n);
        if (n > 1) p[0] = p[1], p[1] = '.';
        char *q = p + 1 + frac;
        q[0] = 'e', q[1] = e < 0 ? '-' : '+';
        if (en == 3) q[2] = (char)('0' + ea / 100);
        q[en] = (char)('0' + ea / 10 % 10), q[en + 1] = (char)('0' + ea % 10);
    }
    return neg + 1 + frac + 2 + en;
}

CSVF_FN int f32_len(uint32_t bits) { return f32_text<false>(nullptr, bits); }
CSVF_FN int f32_put(char *p, uint32_t bits) { return f32_text<true>(p, bits); }

// "frame,class,id,x,y,z\n".  PUT false: only the length.
template <bool PUT>
CSVF_FN int line_text(char *p, int64_t frame, int64_t cls, int64_t id, uint32_t x, uint32_t y, uint32_t z) {
    int n = 0;
    n += PUT ? int_put(p + n, frame) : int_len(frame);
    if (PUT) p[n] = ',';
    ++n;
    n += PUT ? int_put(p + n, cls) : int_len(cls);
    if (PUT) p[n] = ',';
    ++n;
    n += PUT ? int_put(p + n, id) : int_len(id);
    if (PUT) p[n] = ',';
    ++n;
    n += f32_text<PUT>(p + n, x);
    if (PUT) p[n] = ',';
    ++n;
    n += f32_text<PUT>(p + n, y);
    if (PUT) p[n] = ',';
    ++n;
    n += f32_text<PUT>(p + n, z);
    if (PUT) p[n] = '\n';
    return n + 1;
}

CSVF_FN int line_len(int64_t frame, int64_t cls, int64_t id, uint32_t x, uint32_t y, uint32_t z) {
    return line_text<false>(nullptr, frame, cls, id, x, y, z);
}
CSVF_FN int line_put(char *p, int64_t frame, int64_t cls, int64_t id, uint32_t x, uint32_t y, uint32_t z) {
    return line_text<true>(p, frame, cls, id, x, y, z);
}

}  // namespace csvf
