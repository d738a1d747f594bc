// Search for regular expressions: the integer core of k_findrx_count / k_findrx_emit
// (k_findrx.hip), shared with the host code (kolm_reader.cpp) and with the CPU emulation
// tools/findrx_emu.cpp (which walks the same tiles, threads and positions serially and records
// every load).  Tiles, windows, the records, the hold-back and the emit cut are find_core.h's.
//
// The expressions of a call are one deterministic automaton (kolm/regex.py compiles it):
//   cls     256 bytes: the class of every byte value, each < ncls
//   T       nstates x ncls transitions (u16), row-major: T[s * ncls + c]
//   states  0 is dead, 1 is accept; both are absorbing and their rows are all zero (a walk stops
//           on reaching either, so the rows are never read); every other state is >= 2
//   starts  one state per expression, each in [2, nstates): no expression matches the empty string
// Position o matches expression i iff the walk
//       s = starts[i];
//       for (k = 0; k < MAX_WALK && o + k < n; ++k) { s = T[s * ncls + cls[data[o + k]]]; if (s <= 1) break; }
// ends with s == 1, and lo <= o < shi.  The loop bound is unconditional: no table makes a walk
// longer than MAX_WALK steps, and a witness longer than MAX_WALK bytes is no match.
// validate() runs on the host before any launch; with what it accepts, s * ncls + c stays below
// nstates * ncls <= MAX_ENTRIES for every s a walk can hold and every c the map can give, so no
// table the ABI accepts lets a kernel index outside its LDS image.
// hold_back() is the L of find_core.h's group loop, derived from the table alone: the number of
// steps after which no walk is still running, MAX_WALK when there is no smaller bound.
//
// A workgroup stages its tile: the STAGE_WORDS aligned 16-byte words that hold the bytes
// [tile * TILE, tile * TILE + TILE + MAX_WALK - 1) of the buffer, translated to class ids on the
// way (stage_word), so that a step of a walk is one dependent read of the table.  Byte o of the
// buffer is stage byte mis + o - tile * TILE.
// Load contract: find_core.h's (an aligned 16-byte word that holds a byte of [buf, buf + n); a
// word that holds none is not loaded and counts as zeros).  What a word holds outside
// [buf, buf + n) is translated and staged but never walked over: every step tests o + k < n.
#pragma once
#include <cstdio>

#include "find_core.h"

namespace frx {

using fnd::i64;
using fnd::u32;
using fnd::u64;
using fnd::u8;
typedef uint16_t u16;

constexpr u32 MAX_ENTRIES = 16384;        // KOLM_RX_MAX_ENTRIES: nstates * ncls of a call (32 KiB of LDS)
constexpr u32 MAX_WALK = fnd::MAX_LEN;    // steps of a walk = bytes of the longest witness
constexpr u32 MAP = 256;                  // bytes of the class map
// words of a tile's stage: mis <= 15 bytes in front, TILE positions, MAX_WALK - 1 bytes behind
constexpr u32 STAGE_WORDS = (fnd::WORD - 1 + fnd::TILE + MAX_WALK - 1 + fnd::WORD - 1) / fnd::WORD;
constexpr u32 STAGE_BYTES = STAGE_WORDS * fnd::WORD;

struct Starts {
    u16 s[fnd::MAX_PATTERNS];
};

// u16 entries of the table as the device holds it: whole 16-byte words, zeros behind the last row
inline u32 padded_entries(u32 nstates, u32 ncls) { return (nstates * ncls + 7u) & ~7u; }

// Null when the automaton is one the kernels may walk; otherwise msg (what is wrong with it).
inline const char* validate(const u8* cls, const u16* T, u32 nstates, u32 ncls, const u16* starts, u32 np, char* msg,
                            size_t cap) {
    if (np < 1 || np > fnd::MAX_PATTERNS) {
        snprintf(msg, cap, "%u expressions (1..%u are allowed)", np, fnd::MAX_PATTERNS);
        return msg;
    }
    if (!cls || !T || !starts) {
        snprintf(msg, cap, "a null table");
        return msg;
    }
    if (ncls < 1 || ncls > 256 || nstates < 3 || (u64)nstates * ncls > MAX_ENTRIES) {
        snprintf(msg, cap, "%u states x %u classes (1..256 classes, at least 3 states, at most %u entries)", nstates, ncls,
                 MAX_ENTRIES);
        return msg;
    }
    for (u32 b = 0; b < MAP; ++b)
        if (cls[b] >= ncls) {
            snprintf(msg, cap, "byte %u has class %u of %u", b, (u32)cls[b], ncls);
            return msg;
        }
    for (u32 x = 0; x < nstates * ncls; ++x) {
        if (x < 2 * ncls ? T[x] != 0 : T[x] >= nstates) {
            snprintf(msg, cap, "entry %u of state %u is %u (rows 0 and 1 are zero, every entry is below %u)", x % ncls,
                     x / ncls, (u32)T[x], nstates);
            return msg;
        }
    }
    for (u32 i = 0; i < np; ++i)
        if (starts[i] < 2 || starts[i] >= nstates) {
            snprintf(msg, cap, "expression %u starts in state %u (2..%u: the dead and the accepting state start nothing)", i,
                     (u32)starts[i], nstates - 1);
            return msg;
        }
    return nullptr;
}

// The hold-back of a validated automaton: the least L such that every walk has stopped after L
// steps, MAX_WALK when walks can run that long (a cycle among the live states, or a longer path).
// `live` is scratch of nstates bytes x 2.
inline u32 hold_back(const u16* T, u32 nstates, u32 ncls, const u16* starts, u32 np, u8* scratch) {
    u8 *cur = scratch, *nxt = scratch + nstates;
    for (u32 s = 0; s < nstates; ++s) cur[s] = 0;
    for (u32 i = 0; i < np; ++i) cur[starts[i]] = 1;
    for (u32 k = 1; k < MAX_WALK; ++k) {  // cur: the states >= 2 a walk can hold after k - 1 steps
        bool any = false;
        for (u32 s = 0; s < nstates; ++s) nxt[s] = 0;
        for (u32 s = 2; s < nstates; ++s)
            if (cur[s])
                for (u32 c = 0; c < ncls; ++c) {
                    const u32 t = T[s * ncls + c];
                    if (t > 1) nxt[t] = 1, any = true;
                }
        if (!any) return k;
        u8* x = cur;
        cur = nxt, nxt = x;
    }
    return MAX_WALK;
}

// Word w (< STAGE_WORDS) of the stage of `tile`, as class ids: o[q] = stage bytes 16 w + 4 q .. + 3
template <class Ld>
FND_HD void stage_word(Ld& ld, u32 mis, u32 tile, u32 w, u32 n, const u8* cls, u32 o[4]) {
    const i64 off = (i64)tile * fnd::TILE - (i64)mis + (i64)w * fnd::WORD;
    const fnd::Word W = fnd::word_or_zero(ld, off, n);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (u32 q = 0; q < 4; ++q) {
        const u32 x = (u32)(W.q[q >> 1] >> (32 * (q & 1)));
        o[q] = (u32)cls[x & 0xFF] | (u32)cls[(x >> 8) & 0xFF] << 8 | (u32)cls[(x >> 16) & 0xFF] << 16 | (u32)cls[x >> 24] << 24;
    }
}

// bit j: position p0 + j matches the expression that starts in `start`.  sc: the staged class ids
// from position p0 on (MAX_WALK - 1 of them behind the thread's last position).
FND_HD u32 match_mask(const u16* T, u32 ncls, const u8* sc, u32 p0, u32 lo, u32 shi, u32 n, u32 start) {
    const u16* row = T + start * ncls;
    u32 m = 0;
    for (u32 j = 0; j < fnd::PER; ++j) {
        const u32 o = p0 + j;
        if (o < lo || o >= shi || o >= n) continue;
        u32 s = row[sc[j]];
        if (s > 1) {  // on text nearly every walk is dead by now
            const u32 room = n - o < MAX_WALK ? n - o : MAX_WALK;
            for (u32 k = 1; k < room; ++k) {
                s = T[s * ncls + sc[j + k]];
                if (s <= 1) break;
            }
        }
        if (s == 1) m |= 1u << j;
    }
    return m;
}

}  // namespace frx
