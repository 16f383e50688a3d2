/* txq_regex.h — one regular expression as a flat automaton, and the one statement of what "the automaton matches a record"
 * means (`tetrex query --gpu-verify`; not in the reference).  The blob is written by the host
 * (Matcher::export_dfa, txh_regex_automaton of include/txh.h) and read by txq_regex_filter (include/txq.h): the kernel of
 * tetrex_amd/csrc/txq_regex.hip and the host twin txh_regex_filter both step through txq_regex_step below, the way
 * txq_exec_plan.hpp is shared between a CPU test and the executor's kernels.
 *
 * The automaton is the deterministic, unanchored "contains" automaton of a pattern: run over a record from its first byte,
 * it reaches the accept state as soon as some match of the pattern ends at the byte just read.  `^` and `$` are the record's
 * ends, which is why there are two start states and a second flag.
 *
 * Layout (little endian, no pointers; a blob starts at a multiple of 16 bytes wherever it is kept):
 *     u32 magic          TXQ_REGEX_MAGIC
 *     u32 n_states       2 .. 65535; state 0 is the dead state, state 1 the accept state, both absorbing
 *     u32 n_classes      1 .. 256
 *     u32 start_begin    the state in front of a record's first byte
 *     u32 start_mid      the state a scan starts in that begins behind the record's first byte
 *     u32 lmax           the longest match in bytes; TXQ_REGEX_UNBOUNDED where the pattern has `*`, `+` or `{m,}`
 *     u32 total_bytes    TXQ_REGEX_BYTES(n_states, n_classes): header, tables and padding to a multiple of 16
 *     u32 reserved       0
 *     u8  class_of[256]  byte -> class
 *     u16 next[n_states][n_classes]
 *     u8  flags[n_states]    bit 0: accepts here (state 1 only), bit 1: accepts if the record ends here
 *
 * A record of n bytes matches when, with s = start_begin and s = next[s][class_of[b]] for its bytes b in order, s becomes 1
 * at some point (start_begin itself may be 1: the pattern matches the empty string), or flags[s] has bit 1 set after the last
 * byte.  Since both 0 and 1 are absorbing no sentinel is needed, and "became 1" may be tested as late as one likes. */
#ifndef TXQ_REGEX_H
#define TXQ_REGEX_H
#include <stddef.h>
#include <stdint.h>

#define TXQ_REGEX_MAGIC 0x58525854u /* "TXRX" */
#define TXQ_REGEX_UNBOUNDED 0xFFFFFFFFu
#define TXQ_REGEX_MAX_STATES 65535u
#define TXQ_REGEX_HEADER 32u
#define TXQ_REGEX_TABLES (TXQ_REGEX_HEADER + 256u) /* offset of next[][] */
#define TXQ_REGEX_BYTES(n_states, n_classes) \
    ((TXQ_REGEX_TABLES + (size_t)(n_states) * (size_t)(n_classes) * 2u + (size_t)(n_states) + 15u) & ~(size_t)15u)
#define TXQ_REGEX_DEAD 0u
#define TXQ_REGEX_ACCEPT 1u

#ifdef __cplusplus
#if defined(__HIPCC__)
#define TXQ_REGEX_HD __host__ __device__ inline
#else
#define TXQ_REGEX_HD inline
#endif

/* A blob, opened: the header's fields and where the tables are.  `base` may point to any memory the caller can read (the
 * kernel opens the same blob in LDS or in the arena). */
struct txq_regex_view {
    const uint8_t* class_of;
    const uint16_t* next;
    const uint8_t* flags;
    uint32_t n_states, n_classes, start_begin, start_mid, lmax, total_bytes;
};

TXQ_REGEX_HD uint32_t txq_regex_u32(const uint8_t* p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

/* The header's fields from eight words (the kernel reads them with word loads), checked against `avail` bytes: false when
 * the blob is malformed or does not fit.  Transitions and classes are not walked here: txq_regex_step clamps what it reads. */
TXQ_REGEX_HD bool txq_regex_header(const uint32_t h[8], size_t avail, txq_regex_view* v) {
    if (avail < TXQ_REGEX_TABLES || h[0] != TXQ_REGEX_MAGIC) return false;
    v->n_states = h[1], v->n_classes = h[2], v->start_begin = h[3], v->start_mid = h[4], v->lmax = h[5], v->total_bytes = h[6];
    if (v->n_states < 2 || v->n_states > TXQ_REGEX_MAX_STATES || v->n_classes < 1 || v->n_classes > 256) return false;
    if (v->start_begin >= v->n_states || v->start_mid >= v->n_states) return false;
    if ((size_t)v->total_bytes != TXQ_REGEX_BYTES(v->n_states, v->n_classes) || (size_t)v->total_bytes > avail) return false;
    return true;
}

/* the tables of a blob that starts at `base` (any copy of it) */
TXQ_REGEX_HD void txq_regex_bind(txq_regex_view* v, const uint8_t* base) {
    v->class_of = base + TXQ_REGEX_HEADER;
    v->next = reinterpret_cast<const uint16_t*>(base + TXQ_REGEX_TABLES);
    v->flags = base + TXQ_REGEX_TABLES + (size_t)v->n_states * v->n_classes * 2u;
}

TXQ_REGEX_HD bool txq_regex_open(const uint8_t* blob, size_t avail, txq_regex_view* v) {
    if (!blob || avail < TXQ_REGEX_TABLES || ((uintptr_t)blob & 1)) return false;
    uint32_t h[8];
    for (int i = 0; i < 8; ++i) h[i] = txq_regex_u32(blob + 4 * i);
    if (!txq_regex_header(h, avail, v)) return false;
    txq_regex_bind(v, blob);
    return true;
}

/* One byte.  A class or a state outside the tables (a blob nobody checked) reads as class 0 / the dead state, so no load
 * leaves the blob whatever it holds. */
TXQ_REGEX_HD uint32_t txq_regex_step(const txq_regex_view& v, uint32_t state, uint8_t byte) {
    uint32_t c = v.class_of[byte];
    c = c < v.n_classes ? c : 0u;
    const uint32_t to = v.next[state * v.n_classes + c];
    return to < v.n_states ? to : TXQ_REGEX_DEAD;
}

TXQ_REGEX_HD bool txq_regex_accepts_at_end(const txq_regex_view& v, uint32_t state) {
    return state == TXQ_REGEX_ACCEPT || (v.flags[state] & 2u) != 0;
}

/* Does the automaton match the record bytes[0 .. n)?  (false for a blob txq_regex_open refuses) */
TXQ_REGEX_HD bool txq_regex_view_matches(const txq_regex_view& v, const uint8_t* bytes, size_t n) {
    uint32_t s = v.start_begin;
    for (size_t i = 0; i < n && s > TXQ_REGEX_ACCEPT; ++i) s = txq_regex_step(v, s, bytes[i]);
    return txq_regex_accepts_at_end(v, s);
}

TXQ_REGEX_HD bool txq_regex_record_matches(const uint8_t* blob, const uint8_t* bytes, size_t n) {
    txq_regex_view v;
    if (!txq_regex_open(blob, blob ? (size_t)txq_regex_u32(blob + 24) : 0, &v)) return false;
    return txq_regex_view_matches(v, bytes, n);
}
#endif /* __cplusplus */
#endif /* TXQ_REGEX_H */
