/*
 * hsg_eval_text.h -- C ABI of the evaluation step's word ids FROM ARTICLE BYTES (libhsg.so,
 * gfx950).  include/hsg_eval_words.h's hsg_eval_select_words blocks n-grams on document-local
 * word ids; this header makes those ids on the device.  The host hands over the sentences'
 * UTF-8 bytes and splits nothing: the device splits every row at Python's `str.split()`
 * whitespace and gives equal words of a document equal ids, in the layout (word_ptr, word_ids)
 * that hsg_eval_select_words reads.  Ids are only ever compared with each other
 * (hsg_eval_words.h: "no id is invalid"), so the id of a word is simply the position of the
 * document's first word with the same bytes.
 *
 * These entry points live in the same libhsg.so as include/hsg.h's, in a header of their own
 * (as hsg_train.h, hsg_model.h, hsg_embed.h, hsg_eval.h and hsg_eval_words.h).  This header
 * carries the same two obligations itself: its declarations equal its entry in the binding's
 * registry, _lib.ABI["hsg_eval_text.h"] (tests/test_abi_conformance.py), and every entry point
 * below that writes through a pointer has
 * a guard-band case in tests/test_gpu_eval_text_guard.py.
 *
 * Conventions are hsg.h's: device pointers, caller-owned buffers, no allocation, no
 * synchronisation, no global mutable state, `stream` (a hipStream_t as void*) last, every
 * call graph-capturable; 0 on success, a hipError_t, or HSG_EINVAL before any launch.
 */
#ifndef HSG_EVAL_TEXT_H_
#define HSG_EVAL_TEXT_H_

#include <stddef.h>
#include <stdint.h>

#include "hsg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* hsg_eval_text_supported (host-only): 0 <= n <= 2^20 rows, 1 <= B <= 2^20 documents,
 * 0 <= nbytes <= 2^30. */
int hsg_eval_text_supported(int n, int B, int64_t nbytes);

/* hsg_eval_text_word_bound (host-only): (nbytes + n) / 2, the most words n rows that share
 * nbytes bytes can have: a row of L bytes has at most ceil(L / 2) words, since two words are at
 * least one whitespace byte apart.  0 for arguments hsg_eval_text_supported declines. */
int64_t hsg_eval_text_word_bound(int n, int64_t nbytes);

/* hsg_eval_text_workspace_bytes (host-only): the size of `ws` below, 4 * (4 * bound + B + 1)
 * with bound = hsg_eval_text_word_bound(n, nbytes): every word's first byte and length, two
 * table slots per word, and the documents' row ranges.  0 for arguments
 * hsg_eval_text_supported declines. */
size_t hsg_eval_text_workspace_bytes(int n, int B, int64_t nbytes);

/* ---- split and intern ------------------------------------------------------------------------
 * Inputs.
 *   text uint8 [nbytes]: the rows' bytes, concatenated in row order (NULL only if nbytes == 0).
 *   byte_ptr int32 [n+1]: row i owns text[byte_ptr[i] .. byte_ptr[i+1]).  Every value is clamped
 *     to [0, nbytes] and an end below its start is an empty row, so nothing outside text is read
 *     whatever byte_ptr holds (the rules of word_ptr in hsg_eval_words.h).
 *   doc_off int32 [B+1], as in hsg_eval_select_words.  Interning needs every row in exactly one
 *     document, whatever doc_off holds, so only the inner boundaries are used: with e_0 = 0,
 *     e_d = max(e_{d-1}, clamp(doc_off[d], 0, n)) for 0 < d < B and e_B = n, document d owns the
 *     rows e_d .. e_{d+1}-1.  For a doc_off that ascends from 0 to n these are doc_off's own
 *     documents.
 *
 * Whitespace is stated on raw bytes, so it is defined for any input, valid UTF-8 or not.  A
 * whitespace sequence is one of
 *     09..0D, 1C..1F, 20                       U+0009-000D, U+001C-001F, U+0020
 *     C2 85, C2 A0                             U+0085, U+00A0
 *     E1 9A 80                                 U+1680
 *     E2 80 {80..8A, A8, A9, AF}               U+2000-200A, U+2028, U+2029, U+202F
 *     E2 81 9F                                 U+205F
 *     E3 80 80                                 U+3000
 * the UTF-8 forms of the 29 code points at which Python's str.split() splits.  A sequence must
 * lie wholly inside its row: a truncated one at a row's end is not whitespace and never joins
 * with the next row's bytes.  No sequence starts inside another (no first byte is a
 * continuation byte), so "covered by a sequence" is a function of a byte's five neighbours.
 *
 * Words.  A word is a maximal run of bytes of one row that no whitespace sequence covers.  For
 * a str s, the words of s.encode("utf-8", "surrogatepass") are the encoded pieces of s.split().
 *
 * Outputs.
 *   word_ptr int32 [n+1], dense in row order: word_ptr[0] = 0 and word_ptr[i+1] - word_ptr[i]
 *     is the number of words of row i.
 *   word_ids int32 [word_cap]: word_ids[k] is the smallest position k' <= k of a word of the
 *     SAME document whose bytes are identical (same length, same bytes).  The ids are a pure
 *     function of the input: bitwise reproducible, independent of scheduling, bit-exact against
 *     a numpy restatement (tests/eval_text_ref.py).  Entries at and beyond word_ptr[n] are not
 *     written.
 *   word_cap must be at least hsg_eval_text_word_bound(n, nbytes), which covers every byte_ptr
 *     whose rows do not overlap: nothing is refused at run time.  Rows that overlap (a byte_ptr
 *     that does not ascend) can have more words than the bound; then every word_ptr value is
 *     capped at the bound and the words beyond it are dropped, so nothing outside the buffers
 *     is touched.
 *   ws: hsg_eval_text_workspace_bytes(n, B, nbytes) bytes, 4-byte aligned, initialised by the
 *     call itself; its contents afterwards are unspecified.
 *
 * HSG_EINVAL before any launch: arguments hsg_eval_text_supported declines, word_cap below the
 * bound, a NULL byte_ptr, doc_off, word_ptr or ws, NULL text with nbytes > 0, NULL word_ids
 * with a bound > 0.  n == 0 still writes word_ptr[0] = 0.
 *
 * Shape: four launches on `stream`, no host read-back between them nor before the selection.
 *   count   one wave per row: a lane decides from its byte's neighbours whether a word starts
 *           there; the row's count is the popcount of the 64-bit ballots.
 *   scan    one block: word_ptr from the counts, and the documents' row ranges e_d.
 *   emit    one wave per row: each word's first byte and length go to ws at its position.
 *   intern  one block per document, one thread per word, over an open-addressing table of two
 *           slots per word of the document in ws.  A slot holds the smallest position seen so
 *           far of one byte string (claimed with atomicCAS, lowered with atomicMin: at every
 *           moment its representative is byte-equal); membership is decided by comparing bytes,
 *           never by the hash alone; every probe loop is bounded by the table size; integer
 *           atomics only.  After a block barrier every word reads its slot's final value.
 * Its cost is latency over a few hundred KB, not bandwidth. */
int hsg_eval_text_words(int n, int B, const uint8_t *text, int64_t nbytes, const int32_t *byte_ptr,
                        const int32_t *doc_off, int64_t word_cap, int32_t *word_ptr, int32_t *word_ids, void *ws,
                        void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HSG_EVAL_TEXT_H_ */
