// handle_common.h — the front of a qp_ballot_box_* / qp_ledger_* call, worded
// once for both handles (ballot.cpp, ledger.cpp): the refusals that differ by the
// handle's nouns alone, the error of a call that has no handle to carry it, and
// the verify-and-gather front of *_cast, and the three calls on the log
// commitment, and the two on the nullifier-set commitment.  H is a handle with
// err, dead, ctx, admitted(), cap(), its LogCommit lc, its SetCommit sc and the nouns H::HANDLE ("box"), H::ENTRY ("ballot") and H::ABI
// ("qp_ballot_box").  fn names the ABI call in the text.  A text that differs
// by more than the nouns stays with its handle.
#pragma once
#include <stdint.h>
#include <string.h>
#include <new>
#include <string>
#include <vector>
#include "../../include/qpgpu.h"
#include "ctx.h"
#include "slot_table.h"
#include "verifier.h"

namespace qph {

template <class H>
int refuse(H *h, int rc, std::string why) {
  h->err = std::move(why);
  return rc;
}

template <class H>
int dead_handle(H *h, const char *fn) {
  return refuse(h, QP_ERR_STATE, std::string(fn) + ": an earlier call on this " + H::HANDLE +
                                     " failed on the device part-way; its state is not known");
}

template <class H>
int bad_alloc(H *h, const char *fn) {
  return refuse(h, QP_ERR_OOM, std::string(fn) + ": out of host memory");
}

template <class H>
int null_buffer(H *h, const char *fn) {
  return refuse(h, QP_ERR_ARG, std::string(fn) + ": null buffer");
}

// a failed device step leaves the handle dead, as a failed cast does
template <class H>
int device_step(H *h, int rc) {
  if (rc) h->dead = true;
  return rc;
}

// seqs[k] all inside the log, or QP_ERR_ARG naming the first that is not
template <class H>
int check_seqs(H *h, const char *fn, const uint64_t *seqs, uint32_t k) {
  for (uint32_t i = 0; i < k; i++)
    if (seqs[i] >= h->admitted())
      return refuse(h, QP_ERR_ARG, std::string(fn) + ": entry " + std::to_string(seqs[i]) + " (position " +
                                       std::to_string(i) + ") is outside the log's " + std::to_string(h->admitted()));
  return QP_OK;
}

template <class H>
int empty_log(H *h, const char *fn) {
  return refuse(h, QP_ERR_STATE, std::string(fn) + ": empty log (no " + H::ENTRY + " has been admitted yet)");
}

// the sizes ms[k] of *_roots_at all in 1..admitted, or QP_ERR_ARG naming the first that is not
template <class H>
int check_sizes(H *h, const char *fn, const uint64_t *ms, uint32_t k) {
  for (uint32_t i = 0; i < k; i++)
    if (!ms[i] || ms[i] > h->admitted())
      return refuse(h, QP_ERR_ARG, std::string(fn) + ": size " + std::to_string(ms[i]) + " (position " + std::to_string(i) +
                                       ") is outside 1.." + std::to_string(h->admitted()) + ", the sizes the log has had");
  return QP_OK;
}

// the range [first, first + k) of *_entries inside the log
template <class H>
int check_range(H *h, const char *fn, uint64_t first, uint64_t k) {
  if (first > h->admitted() || k > h->admitted() - first)
    return refuse(h, QP_ERR_ARG, std::string(fn) + ": entries [" + std::to_string(first) + ", " + std::to_string(first) +
                                     " + " + std::to_string(k) + ") are outside the log's " + std::to_string(h->admitted()));
  return QP_OK;
}

// keys[k][4] (`what`: "nullifier", "account") all canonical field elements
template <class H>
int canonical_keys(H *h, const char *fn, const char *what, const uint64_t *keys, uint32_t k) {
  for (uint32_t i = 0; i < k; i++)
    for (uint32_t f = 0; f < 4; f++)
      if (keys[(size_t)i * 4 + f] >= qst::P)
        return refuse(h, QP_ERR_ARG, std::string(fn) + ": " + what + " at position " + std::to_string(i) + " felt " +
                                         std::to_string(f) + " is not a canonical field element");
  return QP_OK;
}

// a batch that admits k more than the capacity holds
template <class H>
int over_capacity(H *h, const char *fn, uint64_t k) {
  return refuse(h, QP_ERR_ARG, std::string(fn) + ": " + std::to_string(h->admitted()) + " + " + std::to_string(k) +
                                   " admitted " + H::ENTRY + "s exceed the capacity " + std::to_string(h->cap()) +
                                   "; call " + H::ABI + "_reserve first");
}

// what *_reserve refuses: a capacity that is 0, above 2^31 or below the admitted count
template <class H>
int check_reserve(H *h, const char *fn, uint64_t new_capacity) {
  if (new_capacity > qst::MAX_CAPACITY || new_capacity < h->admitted() || !new_capacity)
    return refuse(h, QP_ERR_ARG, std::string(fn) + ": capacity " + std::to_string(new_capacity) + " for " +
                                     std::to_string(h->admitted()) + " admitted " + H::ENTRY +
                                     "s: it must hold them (and at least one) and be at most 2^31");
  return QP_OK;
}

// The reason of a call that has no handle to carry it (*_new, *_restore, *_log_audit): what
// *_last_error(NULL) returns on this thread, and c's err when there is a context.  Each handle's
// .cpp holds one, thread_local.
struct HandlelessError {
  std::string text;
  void set(qp_ctx *c, const std::string &why) {
    text = why;
    if (c) c->err = why;
  }
};

// The front of *_cast, before n and the buffers are looked at: the verifier's circuit has the
// handle's npi public inputs; circuit: the words for whose those are ("a voting circuit's").
template <class H>
int check_verifier(H *h, const char *fn, qp_verifier *v, uint32_t want, const char *circuit) {
  const uint32_t npi = qv::public_input_count(v);
  if (npi == want) return QP_OK;
  return refuse(h, QP_ERR_ARG,
                std::string(fn) + (!v     ? ": null verifier"
                                   : !npi ? ": the verifier is not usable"
                                          : ": the verifier's circuit has " + std::to_string(npi) + " public inputs; " +
                                                circuit + " has " + std::to_string(want)));
}

// the rest of it: the n proofs verified, verdicts[n], and pis[n][npi] = the public inputs of the
// accepted ones (zero for the others), for the handle's cast_screened
template <class H>
int verify_and_gather(H *h, const char *fn, qp_verifier *v, const uint8_t *const *proofs, const size_t *lens, uint32_t n,
                      uint32_t npi, std::vector<uint32_t> &verdicts, std::vector<uint64_t> &pis) {
  verdicts.assign(n, 0);
  if (const int rc = qp_verifier_verify(v, proofs, lens, n, verdicts.data()))
    return refuse(h, rc, std::string(fn) + ": qp_verifier_verify: " + qp_verifier_last_error(v));
  pis.assign((size_t)n * npi, 0);
  for (uint32_t i = 0; i < n; i++)
    if (verdicts[i] == QP_VERIFY_OK) memcpy(&pis[(size_t)i * npi], qv::public_inputs(v, proofs[i]), (size_t)npi * 8);
  return QP_OK;
}

// ---- *_commit_log, *_receipts and *_roots_at.  commit(h): the handle's commit on either path (its
// leaf kernel, its error word's text and code); the log is not empty when it is called.

// brings the commitment up to date and stores (root, n), either of which may be null
template <class H, class Commit>
int commit_log(H *h, const char *fn, Commit commit, uint64_t root_out[4], uint64_t *n_out) {
  if (!h) return QP_ERR_ARG;
  if (h->dead) return dead_handle(h, fn);
  if (!h->admitted()) return empty_log(h, fn);
  try {
    if (int rc = device_step(h, commit(h))) return rc;
  } catch (const std::bad_alloc &) {
    return bad_alloc(h, fn);
  }
  h->lc.pair(root_out, n_out);
  return QP_OK;
}

template <class H, class Commit>
int receipts(H *h, const char *fn, Commit commit, const uint64_t *seqs, uint32_t k, uint64_t *siblings, uint32_t *path_bits,
             uint32_t *depth, uint64_t *leaves, uint64_t root_out[4], uint64_t *n_out) {
  if (!h) return QP_ERR_ARG;
  if (h->dead) return dead_handle(h, fn);
  if (!h->admitted()) return empty_log(h, fn);
  if (k && (!seqs || !siblings || !path_bits || !depth)) return null_buffer(h, fn);
  if (int rc = check_seqs(h, fn, seqs, k)) return rc;
  if (int rc = commit_log(h, fn, commit, root_out, n_out)) return rc;
  if (!k) return QP_OK;
  return device_step(h, h->lc.receipts(h->ctx, h->err, seqs, k, siblings, path_bits, depth, leaves));
}

// node: the log's node hash, for the host path
template <class H, class Commit, class NodeHash>
int roots_at(H *h, const char *fn, Commit commit, NodeHash node, const uint64_t *ms, uint32_t k, uint64_t *roots_out) {
  if (!h) return QP_ERR_ARG;
  if (h->dead) return dead_handle(h, fn);
  if (!h->admitted()) return empty_log(h, fn);
  if (k && (!ms || !roots_out)) return null_buffer(h, fn);
  if (int rc = check_sizes(h, fn, ms, k)) return rc;
  if (int rc = commit_log(h, fn, commit, nullptr, nullptr)) return rc;
  if (!k) return QP_OK;
  return device_step(h, h->lc.roots_at(h->ctx, h->err, ms, k, node, roots_out));
}

// ---- *_commit_set and *_set_proofs (set_commit.h; nullifier_set.h has the definitions).
// commit(h): the handle's set commit on either path (its log's nullifier column and member bit, its
// defensive error's text and code).  An empty log has the empty set: (four zeros, 0), no refusal.

// brings the set commitment up to date and stores (root, m), either of which may be null
template <class H, class Commit>
int commit_set(H *h, const char *fn, Commit commit, uint64_t root_out[4], uint64_t *m_out) {
  if (!h) return QP_ERR_ARG;
  if (h->dead) return dead_handle(h, fn);
  try {
    if (int rc = device_step(h, commit(h, fn))) return rc;
  } catch (const std::bad_alloc &) {
    return bad_alloc(h, fn);
  }
  h->sc.pair(root_out, m_out);
  return QP_OK;
}

template <class H, class Commit, class Out>
int set_proofs(H *h, const char *fn, Commit commit, const uint64_t *keys, uint32_t k, const Out &o, uint64_t root_out[4],
               uint64_t *m_out) {
  if (!h) return QP_ERR_ARG;
  if (h->dead) return dead_handle(h, fn);
  bool null = !keys || !o.found || !o.pos;
  for (int sl = 0; sl < 2; sl++) null = null || !o.key[sl] || !o.seq[sl] || !o.sib[sl] || !o.bits[sl] || !o.depth[sl];
  if (k && null) return null_buffer(h, fn);
  if (int rc = canonical_keys(h, fn, "nullifier", keys, k)) return rc;
  if (int rc = commit_set(h, fn, commit, root_out, m_out)) return rc;
  if (!k) return QP_OK;
  try {
    return device_step(h, h->sc.proofs(h->ctx, h->err, keys, k, o));
  } catch (const std::bad_alloc &) {
    return bad_alloc(h, fn);
  }
}

}  // namespace qph
