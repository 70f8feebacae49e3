/* circl_hip.h -- C ABI of libcirclhip.so, the MI355X (gfx950) batch ML-KEM / ML-DSA engine.
 *
 * This is the drop-in boundary for cloudflare/circl's lattice hot path.  The reference has no
 * FFI of its own (it is pure Go + Go assembler), so each entry point below cites the reference
 * Go interface it replaces; INTEGRATION.md shows the cgo binding a CIRCL maintainer would add
 * under kem/mlkem and sign/mldsa.
 *
 * Conventions
 *   - plain pointers and sizes only; the caller owns every buffer; nothing is retained after
 *     return (cgo pointer rule); no exceptions or aborts cross the ABI.
 *   - batches are contiguous row-major arrays: ek[n][EK], m[n][32], ct[n][CT], ss[n][32] ...
 *   - the ABI is deterministic: randomness (kem.Scheme.Encapsulate's 32 random bytes,
 *     kem/mlkem/mlkem768/kyber.go:104-108) stays on the Go side and arrives as `m` / seeds.
 *   - functions return 0 or a negative CIRCL_HIP_E* code; data-dependent, per-item failures
 *     (the reference's kem.ErrPubKey / kem.ErrPrivKey) are written to status[n] and the
 *     item's outputs are zero-filled.
 *   - `device` >= 0 selects one GPU; CIRCL_HIP_ALL_DEVICES (-1) splits the batch into
 *     contiguous shards, one per visible GPU, with no collective (items are independent).
 *     A SMALL call is not split: it goes to ONE device, taken round-robin (a host thread and a launch per device for a
 *     handful of items cost more than they return) -- up to 1024 items for ML-KEM and ML-DSA verification, up to 64 for the
 *     operations whose small batches are latency-bound for hundreds of microseconds (ML-DSA signing and key generation,
 *     X25519 and the hybrids), so that a few hundred of those already use every device.
 *   - the *_dev variants take DEVICE pointers and a hipStream_t (as void*), enqueue the
 *     kernels and return without synchronising: this is what bench.py times with inputs
 *     already resident in HBM.  All device pointers must be 16-byte aligned.
 *     The device the pointers live on must be the calling thread's CURRENT device (hipSetDevice); workspace sizes are
 *     valid for every visible device.  Rows that are not a multiple of 4 bytes (ML-DSA signatures, contexts and
 *     messages) are read as whole aligned dwords: device arrays must have at least 4 bytes of addressable slack
 *     behind their last row (the host-buffer entry points provide it themselves).
 *   - host-buffer entry points accept ANY alignment and ordinary pageable memory (a Go []byte sub-slice): every
 *     device owns a pool of staging slots (page-locked host staging + device staging + a stream each) that a small
 *     per-device thread pool, pinned to the GPU's NUMA node, fills and drains, so H2D, kernels and D2H of
 *     successive chunks overlap and a pageable caller reaches the PCIe-bound rate.  Page-locked caller buffers
 *     (circl_hip_alloc_host / hipHostRegister) are DMA-ed directly.  Entry points are re-entrant: concurrent
 *     callers take different slots.  Staging copies of secret inputs / outputs (seeds, private keys, m, shared
 *     secrets) are wiped before a slot is recycled.  Tuning aids: CIRCL_HIP_HOST_THREADS, CIRCL_HIP_HOST_CHUNK
 *     (log2 items per chunk), CIRCL_HIP_HOST_SLOTS.
 *   - there is NO CPU fallback: without a usable HIP device every compute entry point
 *     returns CIRCL_HIP_ENODEV.
 */
#ifndef CIRCL_HIP_H
#define CIRCL_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CIRCL_HIP_OK 0
#define CIRCL_HIP_EPARAM (-1)   /* unknown parameter set / bad argument */
#define CIRCL_HIP_ENODEV (-2)   /* no HIP device, or device index out of range */
#define CIRCL_HIP_EHIP (-3)     /* a HIP runtime call failed (see circl_hip_last_error) */
#define CIRCL_HIP_ENOMEM (-4)
#define CIRCL_HIP_EWORKSPACE (-5) /* workspace too small / misaligned pointer */
#define CIRCL_HIP_EBUSY (-6)    /* the object has calls in flight (circl_hip_keytable_set_coalesce, _async_start / _stop, _close) */
#define CIRCL_HIP_EAGAIN (-7)   /* a *_submit call found every batch of the queue busy: poll / wait for a ticket, then submit again */

#define CIRCL_HIP_ALL_DEVICES (-1)

/* per-item status codes */
#define CIRCL_HIP_ITEM_OK 0
#define CIRCL_HIP_ITEM_ERR_PUBKEY 1  /* kem.ErrPubKey : pke/kyber/kyber768/internal/cpapke.go:45-55 */
#define CIRCL_HIP_ITEM_ERR_PRIVKEY 2 /* kem.ErrPrivKey: kem/mlkem/mlkem768/kyber.go:219-228 */

/* ---- library / device management ------------------------------------------------------ */
int circl_hip_init(void);               /* idempotent; returns the number of devices or <0 */
int circl_hip_device_count(void);
const char *circl_hip_last_error(void); /* thread-local message for the last CIRCL_HIP_EHIP */
const char *circl_hip_version(void);
/* compute units and NUMA node (-1 unknown) of one device; either pointer may be NULL */
int circl_hip_device_info(int device, int *cus, int *numa_node);
/* Device indices of this ABI are LOGICAL.  By default they are the process's HIP devices.  With the environment variable
 * CIRCL_HIP_LOGICAL_DEVICES=L (read once, at the first call; never fewer than the HIP devices) the library presents L
 * devices, logical device d running on HIP device d mod the HIP device count, each with its own staging pool, copy /
 * compute streams and byte movers: a one-GPU box then executes exactly the host-side code of an L-GPU node
 * (CIRCL_HIP_ALL_DEVICES splits into L contiguous shards driven by L threads), and an 8-GPU node can be driven as 16
 * half-shards.  Returns the HIP device behind a logical one, or CIRCL_HIP_ENODEV. */
int circl_hip_physical_device(int device);

/* ---- sizes (kem.Scheme.PublicKeySize etc., kem/kem.go:33-82; sign/sign.go:48-94) -------- */
size_t circl_hip_mlkem_ek_size(int param); /* 512|768|1024 -> 800|1184|1568, 0 if unknown */
size_t circl_hip_mlkem_dk_size(int param); /*                1632|2400|3168 */
size_t circl_hip_mlkem_ct_size(int param); /*                 768|1088|1568 */
size_t circl_hip_mldsa_pk_size(int param); /* 44|65|87 -> 1312|1952|2592 */
size_t circl_hip_mldsa_sig_size(int param);/*             2420|3309|4627 */
size_t circl_hip_mldsa_sk_size(int param); /*             2560|4032|4896 */

/* ---- ML-KEM, host buffers (what cgo binds) ---------------------------------------------
 * circl_hip_mlkem_encaps: scheme.UnmarshalBinaryPublicKey(ek_i) followed by
 *   scheme.EncapsulateDeterministically(pk_i, m_i) for every i
 *   (kem/mlkem/mlkem768/kyber.go:390-396, :359-370 -> :103-137 EncapsulateTo).
 *   status[i] = CIRCL_HIP_ITEM_ERR_PUBKEY when ek_i holds a coefficient >= q.
 * circl_hip_mlkem_decaps: scheme.UnmarshalBinaryPrivateKey(dk_i) followed by
 *   scheme.Decapsulate(sk_i, ct_i) (kyber.go:398-407 -> :209-230 ; :376-386 -> :144-184).
 *   status[i] = CIRCL_HIP_ITEM_ERR_PRIVKEY when H(ek) != the hash stored in dk_i.  An invalid
 *   ciphertext is NOT an error (implicit rejection).
 * circl_hip_mlkem_keygen: scheme.DeriveKeyPair(seed_i), seed = d || z, 64 bytes
 *   (kyber.go:340-345 -> :57-78 NewKeyFromSeed), keys in MarshalBinary form.
 * status may be NULL.
 */
int circl_hip_mlkem_encaps(int param, const uint8_t *ek, const uint8_t *m, uint8_t *ct, uint8_t *ss,
                           uint8_t *status, size_t n, int device);
int circl_hip_mlkem_decaps(int param, const uint8_t *dk, const uint8_t *ct, uint8_t *ss,
                           uint8_t *status, size_t n, int device);
int circl_hip_mlkem_keygen(int param, const uint8_t *seed64, uint8_t *ek, uint8_t *dk, size_t n,
                           int device);

/* ---- ML-KEM, device-resident ------------------------------------------------------------
 * Same semantics; every pointer is a device pointer on the device `stream` belongs to.
 * `workspace` must hold circl_hip_mlkem_workspace_size(param, n) bytes.  status may NOT be NULL.
 * After a call the workspace still holds per-item intermediates that are as secret as the call's secret inputs (the
 * encryption coins r, the decrypted m'): a caller that hands the memory on should zero it (the host-buffer forms do).
 * circl_hip_mlkem_workspace_size is MONOTONE in n: 129 B per item + 32 KB of matrix scratch per resident workgroup (about
 * 134 MB) + a row cache of 8 KB per item for the first 2^15 items (the small-batch routes; at most 256 MB).  A workspace
 * sized once for the largest batch serves every smaller batch.  A call whose workspace lacks the row cache for its n (but
 * has the first two parts and 128 KB) still succeeds, through the big-batch routes; results are identical either way.
 */
size_t circl_hip_mlkem_workspace_size(int param, size_t n);
int circl_hip_mlkem_encaps_dev(int param, const uint8_t *d_ek, const uint8_t *d_m, uint8_t *d_ct,
                               uint8_t *d_ss, uint8_t *d_status, size_t n, void *d_workspace,
                               size_t workspace_bytes, void *stream);
int circl_hip_mlkem_decaps_dev(int param, const uint8_t *d_dk, const uint8_t *d_ct, uint8_t *d_ss,
                               uint8_t *d_status, size_t n, void *d_workspace,
                               size_t workspace_bytes, void *stream);
int circl_hip_mlkem_keygen_dev(int param, const uint8_t *d_seed64, uint8_t *d_ek, uint8_t *d_dk,
                               size_t n, void *d_workspace, size_t workspace_bytes, void *stream);

/* Shared-key encapsulation: all n items use the ONE encapsulation key at `ek` -- n times
 * scheme.EncapsulateDeterministically(pk, m_i) on one parsed key, the shape of the reference's BenchmarkEncapsulate
 * (kem/schemes/schemes_test.go:28-38), where the cached key amortises A^T and H(ek) (kyber.go:39-43).  Same
 * outputs as circl_hip_mlkem_encaps on n copies of the key; status[i] is the key's verdict for every i. */
int circl_hip_mlkem_encaps_shared(int param, const uint8_t *ek, const uint8_t *m, uint8_t *ct, uint8_t *ss,
                                  uint8_t *status, size_t n, int device);
int circl_hip_mlkem_encaps_shared_dev(int param, const uint8_t *d_ek, const uint8_t *d_m, uint8_t *d_ct,
                                      uint8_t *d_ss, uint8_t *d_status, size_t n, void *d_workspace,
                                      size_t workspace_bytes, void *stream);
/* Shared-key decapsulation: n ciphertexts for the ONE private key at `dk` (n times scheme.Decapsulate(sk, ct_i) on one
 * parsed key).  status[i] = 2 (kem.ErrPrivKey) for every i if the key fails its hash check. */
int circl_hip_mlkem_decaps_shared(int param, const uint8_t *dk, const uint8_t *ct, uint8_t *ss, uint8_t *status,
                                  size_t n, int device);
int circl_hip_mlkem_decaps_shared_dev(int param, const uint8_t *d_dk, const uint8_t *d_ct, uint8_t *d_ss,
                                      uint8_t *d_status, size_t n, void *d_workspace, size_t workspace_bytes,
                                      void *stream);

/* ---- ML-KEM key tables (grouped keys) -----------------------------------------------------------
 * A batch over a handful of distinct keys: item i uses row key_idx[i] of a table of nkeys keys.  This is the
 * reference's parsed-key object applied to a batch: kem.Scheme.UnmarshalBinaryPublicKey expands A^T and H(ek) once
 * per KEY (kem/mlkem/mlkem768/kyber.go:39-43, :247-263; pke/kyber/kyber768/internal/cpapke.go:19-25) and every later
 * EncapsulateDeterministically / Decapsulate on that object reuses them.  Here: matrix expansion, H(ek) and the
 * private key's hash check once per TABLE ENTRY, then the shared-key work per item.  Results are identical to
 * circl_hip_mlkem_encaps / _decaps on the gathered rows ek_table[key_idx[i]] / dk_table[key_idx[i]]; status[i] is the
 * verdict of item i's key.  Host entry points return CIRCL_HIP_EPARAM for an index >= nkeys; the _dev variants
 * bound d_key_idx (4-byte aligned) to the table -- an index >= nkeys uses the last entry -- and need
 * circl_hip_mlkem_keyed_workspace_size(param, n, nkeys) bytes. */
int circl_hip_mlkem_encaps_keyed(int param, const uint8_t *ek_table, size_t nkeys, const uint32_t *key_idx,
                                 const uint8_t *m, uint8_t *ct, uint8_t *ss, uint8_t *status, size_t n, int device);
int circl_hip_mlkem_decaps_keyed(int param, const uint8_t *dk_table, size_t nkeys, const uint32_t *key_idx,
                                 const uint8_t *ct, uint8_t *ss, uint8_t *status, size_t n, int device);
size_t circl_hip_mlkem_keyed_workspace_size(int param, size_t n, size_t nkeys);
int circl_hip_mlkem_encaps_keyed_dev(int param, const uint8_t *d_ek_table, size_t nkeys, const uint32_t *d_key_idx,
                                     const uint8_t *d_m, uint8_t *d_ct, uint8_t *d_ss, uint8_t *d_status, size_t n,
                                     void *d_workspace, size_t workspace_bytes, void *stream);
int circl_hip_mlkem_decaps_keyed_dev(int param, const uint8_t *d_dk_table, size_t nkeys, const uint32_t *d_key_idx,
                                     const uint8_t *d_ct, uint8_t *d_ss, uint8_t *d_status, size_t n,
                                     void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- key tables that LIVE ACROSS CALLS: the reference's parsed key objects ----------------------
 * kem.Scheme.UnmarshalBinaryPublicKey / UnmarshalBinaryPrivateKey return objects that keep A^T and H(ek) (kem/mlkem/mlkem768/
 * kyber.go:39-43, :247-263; the private key's hash check :219-228 happens there); sign.Scheme.UnmarshalBinaryPublicKey keeps A
 * and tr (sign/mldsa/mldsa65/internal/dilithium.go:114-126).  A circl_hip_keytable is that cache for nkeys keys, built ONCE on
 * one device: the key bytes, the expanded matrices and the hashes stay resident, and a call moves only its per-item data.
 * Item i of a call uses entry key_idx[i]; key_idx == NULL: every item uses entry 0 (a table of one key = one key object).
 * Results are identical to the per-call key-table entry points above.  A Go bridge keeps one table per key object (or per
 * key set) and frees it from the object's finalizer; a table is immutable and may be used by concurrent calls.
 *   circl_hip_mlkem_keytable_new : private_keys = 0: rows are encapsulation keys; 1: decapsulation keys, whose stored-hash
 *       verdicts (0 | 2 = kem.ErrPrivKey) are written to key_status[nkeys] if it is not NULL.  A public key's canonicity is
 *       reported per item by the encapsulation (status 1 = kem.ErrPubKey), as everywhere in this ABI.
 *   _dev variants: pointers are device memory on the TABLE's device; workspace = circl_hip_mlkem_workspace_size(param, n) /
 *       circl_hip_mldsa_workspace_size(param, n) bytes (no table tail: the table brings its own).  Like every keyed _dev entry point
 *       they cannot REPORT a bad d_key_idx (the host forms check it: an index >= nkeys is CIRCL_HIP_EPARAM; a device array cannot be
 *       checked without a synchronisation), so the kernels BOUND it: an index >= nkeys uses the table's LAST entry -- never memory
 *       behind the table.
 *   circl_hip_keytable_free wipes the key rows of a private table before releasing them.
 *   device = CIRCL_HIP_ALL_DEVICES in any *_new below REPLICATES the table: it is built once on every device, and the host-buffer
 *       *_table calls then split a batch into contiguous shards, one per device, like every other entry point (a table made for
 *       one device runs its calls there).  The _dev variants use the replica on the calling thread's current device;
 *       circl_hip_keytable_on_device returns that replica (or the table itself if it lives on `device`, else NULL) and
 *       circl_hip_keytable_device the table's device (CIRCL_HIP_ALL_DEVICES for a replicated one; CIRCL_HIP_ENODEV for NULL or a
 *       freed table), circl_hip_keytable_nkeys its number of entries (0 likewise). */
typedef struct circl_hip_keytable circl_hip_keytable;
int circl_hip_keytable_device(const circl_hip_keytable *table);
size_t circl_hip_keytable_nkeys(const circl_hip_keytable *table);
const circl_hip_keytable *circl_hip_keytable_on_device(const circl_hip_keytable *table, int device);
int circl_hip_mlkem_keytable_new(int param, int private_keys, const uint8_t *keys, size_t nkeys, int device,
                                 uint8_t *key_status, circl_hip_keytable **out);
int circl_hip_mldsa_keytable_new(int param, const uint8_t *pks, size_t nkeys, int device, circl_hip_keytable **out);
/* ONE ML-DSA private key prepared once -- A and the NTT-domain s1, s2, t0 of the reference's parsed PrivateKey (sign/mldsa/mldsa65/
 * internal/dilithium.go:149-179) -- then any number of scheme.Sign calls with it: circl_hip_mldsa_sign_table[_dev] = circl_hip_mldsa_
 * sign_shared[_dev] without the per-call ExpandA and transforms (workspace: circl_hip_mldsa_sign_workspace_size(param, n)). */
int circl_hip_mldsa_privkey_new(int param, const uint8_t *sk, int device, circl_hip_keytable **out);
/* ... and a table of nkeys prepared private keys (a signer that holds several identities): message i is signed with entry
 * key_idx[i]; key_idx == NULL: entry 0.  Same signatures as circl_hip_mldsa_sign on the gathered rows sks[key_idx[i]].  The host
 * form returns CIRCL_HIP_EPARAM for an index >= nkeys; the _dev form bounds d_key_idx (4-byte aligned) to the table (>= nkeys: the last entry). */
int circl_hip_mldsa_privkeys_new(int param, const uint8_t *sks, size_t nkeys, int device, circl_hip_keytable **out);
int circl_hip_mldsa_sign_table_keyed(const circl_hip_keytable *table, const uint32_t *key_idx, const uint8_t *msg_blob, const uint64_t *msg_off,
                                     const uint8_t *ctx_blob, const uint64_t *ctx_off, const uint8_t *rnd, uint8_t *sig, size_t n);
int circl_hip_mldsa_sign_table_keyed_dev(const circl_hip_keytable *table, const uint32_t *d_key_idx, const uint8_t *d_msg_blob,
                                         const uint64_t *d_msg_off, const uint8_t *d_ctx_blob, const uint64_t *d_ctx_off, const uint8_t *d_rnd,
                                         int internal, uint8_t *d_sig, size_t n, void *d_workspace, size_t workspace_bytes, void *stream);
int circl_hip_mldsa_sign_table(const circl_hip_keytable *table, const uint8_t *msg_blob, const uint64_t *msg_off, const uint8_t *ctx_blob,
                               const uint64_t *ctx_off, const uint8_t *rnd, uint8_t *sig, size_t n);
int circl_hip_mldsa_sign_table_dev(const circl_hip_keytable *table, const uint8_t *d_msg_blob, const uint64_t *d_msg_off,
                                   const uint8_t *d_ctx_blob, const uint64_t *d_ctx_off, const uint8_t *d_rnd, int internal, uint8_t *d_sig,
                                   size_t n, void *d_workspace, size_t workspace_bytes, void *stream);
void circl_hip_keytable_free(circl_hip_keytable *table);
int circl_hip_mlkem_encaps_table(const circl_hip_keytable *table, const uint32_t *key_idx, const uint8_t *m, uint8_t *ct,
                                 uint8_t *ss, uint8_t *status, size_t n);
int circl_hip_mlkem_decaps_table(const circl_hip_keytable *table, const uint32_t *key_idx, const uint8_t *ct, uint8_t *ss,
                                 uint8_t *status, size_t n);
int circl_hip_mldsa_verify_table(const circl_hip_keytable *table, const uint32_t *key_idx, const uint8_t *sig,
                                 const uint8_t *msg_blob, const uint64_t *msg_off, const uint8_t *ctx_blob,
                                 const uint64_t *ctx_off, uint8_t *ok, size_t n);
int circl_hip_mlkem_encaps_table_dev(const circl_hip_keytable *table, const uint32_t *d_key_idx, const uint8_t *d_m,
                                     uint8_t *d_ct, uint8_t *d_ss, uint8_t *d_status, size_t n, void *d_workspace,
                                     size_t workspace_bytes, void *stream);
int circl_hip_mlkem_decaps_table_dev(const circl_hip_keytable *table, const uint32_t *d_key_idx, const uint8_t *d_ct,
                                     uint8_t *d_ss, uint8_t *d_status, size_t n, void *d_workspace, size_t workspace_bytes,
                                     void *stream);
int circl_hip_mldsa_verify_table_dev(const circl_hip_keytable *table, const uint32_t *d_key_idx, const uint8_t *d_sig,
                                     const uint8_t *d_msg_blob, const uint64_t *d_msg_off, const uint8_t *d_ctx_blob,
                                     const uint64_t *d_ctx_off, uint8_t *d_ok, size_t n, void *d_workspace,
                                     size_t workspace_bytes, void *stream);

/* ---- many concurrent ONE-ITEM callers: cross-caller coalescing (opt-in, per table) ------------------------------------------
 * The reference's consumers do not batch: kem/hybrid (kem/hybrid/hybrid.go:95-99), kem/xwing (kem/xwing/xwing.go:259,288), hpke
 * (hpke/algs.go:283-285) and every user of kem.Scheme / sign.Scheme call Encapsulate / Decapsulate / Verify with one key and one
 * item (kem/mlkem/mlkem768/kyber.go:347-386, sign/mldsa/mldsa65/dilithium.go:305) from whichever goroutine owns the connection.
 * One such call through a resident table costs a launch and a wait (tens of microseconds) however little the kernel does.
 * circl_hip_keytable_set_coalesce(table, max_items, max_wait_us) lets the small host-buffer *_table calls of CONCURRENT callers
 * (calls of at most max_items / 4 items) share launches: callers copy their rows into an open batch, the first of them flushes it
 * as soon as the device has room for another batch -- so a batch holds exactly the calls that arrived while the previous ones ran,
 * nothing is delayed when the table is idle -- or after max_wait_us microseconds if that is not 0; each caller returns with its own
 * rows.  Results are byte for byte those of the same calls made one by one (same kernels; items are independent).
 *   max_items: largest batch (2 .. 8192; 0 switches coalescing off).  CIRCL_HIP_EBUSY (nothing changed) while calls are in flight
 *   through the table: set it before the table is shared, or retry.  A replicated table coalesces per replica; its small calls (<= 1024
 *   items) go to one replica each, round-robin.  circl_hip_keytable_coalesce_stats: calls and items that joined batches and the
 *   launches they became (items / launches = mean batch).  Served today: circl_hip_mlkem_encaps_table, circl_hip_mlkem_decaps_table,
 *   circl_hip_mldsa_verify_table, circl_hip_mldsa_sign_table / _sign_table_keyed (a server signing one handshake transcript per call),
 *   circl_hip_hybrid_encaps_table / _decaps_table. */
int circl_hip_keytable_set_coalesce(circl_hip_keytable *table, size_t max_items, uint32_t max_wait_us);
/* Lifetime under concurrent callers: circl_hip_keytable_set_coalesce, circl_hip_keytable_async_start / _stop and circl_hip_keytable_close
 * return CIRCL_HIP_EBUSY -- and change nothing -- while a call is inside the table or one of its batches is open or running; nothing is
 * ever freed under a caller.  circl_hip_keytable_close(table) = circl_hip_keytable_free with that verdict (CIRCL_HIP_OK: freed);
 * circl_hip_keytable_free itself waits up to two seconds for the calls inside to return and, should they not, marks the table dead
 * (later calls get CIRCL_HIP_EPARAM) and LEAKS its memory instead of freeing it under them.
 *
 * ---- the ASYNCHRONOUS form: submit / poll, no sleeping thread per call ---------------------------------------------------------
 * The blocking form above holds one OS thread per outstanding call (a goroutine inside a blocking cgo call holds an M: ten thousand
 * concurrent handshakes, hpke/algs.go:283-285 or kem/hybrid/hybrid.go:95-99, would be ten thousand threads), and the sleep + wake of
 * each of them is most of a coalesced call's host cost (profiles/r05_concurrent_final.txt: 7.6 of 13 us).  With
 *   circl_hip_keytable_async_start(table, max_items, max_wait_us, want_eventfd)
 * the table gets a QUEUE served by one library thread per device (the dispatcher): it closes the open batch whenever the device has
 * room -- same group commit as above: a batch holds what arrived while its predecessors ran, nothing waits on an idle device unless
 * max_wait_us says so -- launches it, copies the finished batch's rows STRAIGHT INTO THE SUBMITTERS' OUTPUT BUFFERS, and publishes the
 * batch's completion.  Served: circl_hip_mlkem_encaps_table_submit (public ML-KEM table), circl_hip_mlkem_decaps_table_submit (private
 * ML-KEM table), circl_hip_mldsa_verify_table_submit (ML-DSA public-key table), circl_hip_hybrid_encaps_table_submit / _decaps_table_submit
 * (X-Wing / X25519MLKEM768 / Kyber-X25519 tables: kem/hybrid/hybrid.go:95-99, kem/xwing/xwing.go:259,288 -- one hybrid launch costs an
 * X25519 ladder, ~0.8 ms, whatever it holds: the calls that gain most from sharing it).
 *   *_submit(...same arrays as the blocking call..., n, &ticket): copies the n <= max_items / 4 items' inputs into the open batch, notes
 *       the output pointers and returns AT ONCE: CIRCL_HIP_OK and a ticket; CIRCL_HIP_EAGAIN when every batch of the queue is busy
 *       (nothing was taken: poll, then submit again); CIRCL_HIP_EPARAM for what the blocking call rejects (a NULL required input, a
 *       key index >= nkeys, an unsupported context) or a table without a queue.  The output buffers (and nothing else: inputs are
 *       copied) must stay valid and untouched until the ticket is done.  Results are byte for byte those of the blocking calls; per-
 *       item verdicts (status / ok rows, a bad decapsulation-key entry, a non-canonical public key) arrive in the rows as always.
 *   circl_hip_poll(table, tickets, n, state): state[i] = 1 done, 0 pending, < 0 the ticket's batch failed (a CIRCL_HIP_E* code; its
 *       output rows were zeroed: no shared secret, ok = 0) or the ticket is not one of this table's (CIRCL_HIP_EPARAM); returns how
 *       many are not pending.  One atomic load per ticket, no lock, no system call.  Tickets of one queue complete in the order
 *       they were issued, so a host that keeps its outstanding tickets in a FIFO only ever needs to look at the head.
 *   circl_hip_wait(table, ticket, timeout_us): blocks the calling thread until the ticket is done (returns its state) or timeout_us
 *       microseconds passed (returns 0); timeout_us < 0: no limit.  ONE thread per device is all a host needs to block.
 *   circl_hip_keytable_eventfd(table, replica): with want_eventfd != 0 the queue owns an eventfd(2) (non-blocking, counter semantics)
 *       that the dispatcher adds 1 to after every finished batch -- put it into the host's own epoll / kqueue set and call
 *       circl_hip_poll when it becomes readable; -1 if the table has none.  replica: 0 for a one-device table, the logical device
 *       for a replicated one (one queue and one dispatcher per replica; a submitted call goes to one replica, round-robin, and its
 *       ticket says which: the top byte).
 *   circl_hip_keytable_async_stop(table): flushes and finishes every submitted call, stops the dispatchers, frees the queues
 *       (CIRCL_HIP_EBUSY while a call is inside the table: a *_submit, a circl_hip_poll, a thread blocked in circl_hip_wait); circl_hip_keytable_free does the same on the way.
 * The blocking *_table calls keep working on such a table (they submit and wait), so one table can serve both kinds of caller.
 * A blocking call that is too large for a batch (more than max_items / 4 items, or messages beyond a quarter of a batch's blob
 * area) runs on its own, through the ordinary path, as it does on a table without a queue; only *_submit refuses such a call. */
int circl_hip_keytable_close(circl_hip_keytable *table);
int circl_hip_keytable_async_start(circl_hip_keytable *table, size_t max_items, uint32_t max_wait_us, int want_eventfd);
int circl_hip_keytable_async_stop(circl_hip_keytable *table);
int circl_hip_keytable_eventfd(const circl_hip_keytable *table, int replica);
int circl_hip_mlkem_encaps_table_submit(const circl_hip_keytable *table, const uint32_t *key_idx, const uint8_t *m, uint8_t *ct, uint8_t *ss,
                                        uint8_t *status, size_t n, uint64_t *ticket);
int circl_hip_mlkem_decaps_table_submit(const circl_hip_keytable *table, const uint32_t *key_idx, const uint8_t *ct, uint8_t *ss, uint8_t *status,
                                        size_t n, uint64_t *ticket);
int circl_hip_mldsa_verify_table_submit(const circl_hip_keytable *table, const uint32_t *key_idx, const uint8_t *sig, const uint8_t *msg_blob,
                                        const uint64_t *msg_off, const uint8_t *ctx_blob, const uint64_t *ctx_off, uint8_t *ok, size_t n,
                                        uint64_t *ticket);
int circl_hip_hybrid_encaps_table_submit(const circl_hip_keytable *table, const uint32_t *key_idx, const uint8_t *eseed, uint8_t *ct, uint8_t *ss,
                                         uint8_t *status, size_t n, uint64_t *ticket);
int circl_hip_hybrid_decaps_table_submit(const circl_hip_keytable *table, const uint32_t *key_idx, const uint8_t *ct, uint8_t *ss, uint8_t *status,
                                         size_t n, uint64_t *ticket);
int circl_hip_poll(const circl_hip_keytable *table, const uint64_t *tickets, size_t n, int8_t *state);
int circl_hip_wait(const circl_hip_keytable *table, uint64_t ticket, int64_t timeout_us);
/* ---- the asynchronous form for keys that come WITH the call: circl_hip_queue ------------------------------------------------------
 * A TLS 1.3 server encapsulates once per handshake, to the CLIENT'S ephemeral key (kem/hybrid/hybrid.go:271-300 ->
 * kem/mlkem/mlkem768/kyber.go:359-370): there is no resident table to hang a queue on.  A circl_hip_queue is that queue by itself: one
 * operation, one parameter set, one device, the same dispatcher thread, tickets, poll / wait / eventfd as above.
 *   circl_hip_queue_open(op, param, device, max_items, want_eventfd, &q): op = CIRCL_HIP_QUEUE_MLKEM_ENCAPS / _MLKEM_DECAPS (param 512 / 768 /
 *       1024) or CIRCL_HIP_QUEUE_HYBRID_ENCAPS / _HYBRID_DECAPS (param = the CIRCL_HIP_HYBRID_* scheme); device >= 0.
 *   circl_hip_queue_submit(q, key, in, out0, ss, status, n, &ticket): n <= max_items / 4 items, each with its OWN key row.
 *       encapsulation: key = n encapsulation (public) keys, in = n seeds m (ML-KEM: 32 bytes; hybrids: their eseed), out0 = n ciphertexts;
 *       decapsulation: key = n decapsulation (private) keys, in = n ciphertexts, out0 unused (NULL).
 *       ss = n shared secrets, status = n per-item status bytes (may be NULL).  key and in are copied before the call returns; out0 / ss /
 *       status must stay valid until the ticket is done.  Returns as the *_table_submit calls do (CIRCL_HIP_EAGAIN: poll, submit again).
 *   circl_hip_queue_poll / _wait / _eventfd: as circl_hip_poll / circl_hip_wait / circl_hip_keytable_eventfd.
 *   circl_hip_queue_close: CIRCL_HIP_EBUSY while a call is inside the queue; otherwise finishes every submitted call, then frees.
 * Bytes are those of circl_hip_mlkem_encaps / _decaps / circl_hip_hybrid_encaps / _decaps on the same rows. */
#define CIRCL_HIP_QUEUE_MLKEM_ENCAPS 1
#define CIRCL_HIP_QUEUE_MLKEM_DECAPS 2
#define CIRCL_HIP_QUEUE_HYBRID_ENCAPS 3
#define CIRCL_HIP_QUEUE_HYBRID_DECAPS 4
typedef struct circl_hip_queue circl_hip_queue;
int circl_hip_queue_open(int op, int param, int device, size_t max_items, int want_eventfd, circl_hip_queue **out);
int circl_hip_queue_close(circl_hip_queue *q);
int circl_hip_queue_eventfd(const circl_hip_queue *q);
int circl_hip_queue_stats(const circl_hip_queue *q, uint64_t *calls, uint64_t *items, uint64_t *launches); /* as circl_hip_keytable_coalesce_stats */
int circl_hip_queue_submit(circl_hip_queue *q, const uint8_t *key, const uint8_t *in, uint8_t *out0, uint8_t *ss, uint8_t *status, size_t n,
                           uint64_t *ticket);
int circl_hip_queue_poll(const circl_hip_queue *q, const uint64_t *tickets, size_t n, int8_t *state);
int circl_hip_queue_wait(const circl_hip_queue *q, uint64_t ticket, int64_t timeout_us);
/* The same for the entry points that take their keys WITH the call -- a TLS 1.3 server encapsulates once per handshake, to the
 * client's ephemeral key share (kem/hybrid/hybrid.go:271-300 -> kem/mlkem/mlkem768/kyber.go:359-370): nothing resident to attach a
 * batch to.  circl_hip_set_coalesce(max_items, max_wait_us), process-wide, default off: small calls (<= max_items / 4 items) of
 * circl_hip_mlkem_encaps, circl_hip_mlkem_decaps, circl_hip_mldsa_verify / _verify_internal, circl_hip_hybrid_encaps and
 * circl_hip_hybrid_decaps from concurrent threads share launches per (entry point, parameter set, device); every item still brings
 * its own key, the bytes are those of the un-coalesced calls.  Call it once, before the threads start (later calls only affect
 * (entry point, parameter set, device) combinations that have not been used yet).  circl_hip_set_coalesce(0, 0) switches new joins off
 * AND DRAINS: it returns once no call is inside any process-wide batch (CIRCL_HIP_EBUSY if that takes more than five seconds). */
int circl_hip_set_coalesce(size_t max_items, uint32_t max_wait_us);
int circl_hip_keytable_coalesce_stats(const circl_hip_keytable *table, uint64_t *calls, uint64_t *items, uint64_t *launches);

/* ---- PrivateKey.Public() over a batch -----------------------------------------------------------
 * circl_hip_mlkem_public_from_private: kem/mlkem/mlkem768/kyber.go:323-328 -- the encapsulation key stored inside each
 *   decapsulation key (a strided copy on the host, no device work).
 * circl_hip_mldsa_public_from_private: sign/mldsa/mldsa65/internal/dilithium.go:473-484 -- t = A s1 + s2 recomputed from the
 *   packed private key (ExpandA, NTT, Power2Round), pk = rho || PackT1(t1).  The _dev form needs
 *   circl_hip_mldsa_workspace_size(param, n) bytes. */
int circl_hip_mlkem_public_from_private(int param, const uint8_t *dk, uint8_t *ek, size_t n);
int circl_hip_mldsa_public_from_private(int param, const uint8_t *sk, uint8_t *pk, size_t n, int device);
int circl_hip_mldsa_public_from_private_dev(int param, const uint8_t *d_sk, uint8_t *d_pk, size_t n, void *d_workspace, size_t workspace_bytes,
                                            void *stream);

/* ---- round-3 Kyber ------------------------------------------------------
 * kem/kyber/kyber{512,768,1024}: the pre-standard KEM the reference still ships ("Kyber512/768/1024" in
 * kem/schemes).  param 512 | 768 | 1024; key and ciphertext sizes are those of ML-KEM.  Differences from
 * ML-KEM (kem/kyber/kyber768/kyber.go):
 *   keygen  scheme.DeriveKeyPair(seed64): G(d) without the domain byte                          :60-82
 *   encaps  scheme.EncapsulateDeterministically(pk, seed32): m = H(seed); (K',r) = G(m || H(pk));
 *           K = KDF(K' || H(ct)); key coefficients >= q are reduced, never rejected   :105-154, :248-262
 *   decaps  scheme.Decapsulate(sk, ct): K = KDF((ct' == ct ? K'' : z) || H(ct)); the private key is
 *           not checked                                                               :156-197, :215-232
 * so none of the three has a per-item failure.  Workspace of the _dev variants:
 * circl_hip_mlkem_workspace_size(param, n). */
int circl_hip_kyber_keygen(int param, const uint8_t *seed64, uint8_t *ek, uint8_t *dk, size_t n,
                           int device);
int circl_hip_kyber_encaps(int param, const uint8_t *ek, const uint8_t *seed32, uint8_t *ct,
                           uint8_t *ss, size_t n, int device);
int circl_hip_kyber_decaps(int param, const uint8_t *dk, const uint8_t *ct, uint8_t *ss, size_t n,
                           int device);
int circl_hip_kyber_keygen_dev(int param, const uint8_t *d_seed64, uint8_t *d_ek, uint8_t *d_dk,
                               size_t n, void *d_workspace, size_t workspace_bytes, void *stream);
int circl_hip_kyber_encaps_dev(int param, const uint8_t *d_ek, const uint8_t *d_seed32, uint8_t *d_ct,
                               uint8_t *d_ss, size_t n, void *d_workspace, size_t workspace_bytes,
                               void *stream);
int circl_hip_kyber_decaps_dev(int param, const uint8_t *d_dk, const uint8_t *d_ct, uint8_t *d_ss,
                               size_t n, void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- ML-DSA (param 44 | 65 | 87) and round-3 Dilithium2/3/5 (param 2 | 3 | 5) ----
 * Every circl_hip_mldsa_* entry point below also accepts param 2, 3 or 5 = sign/dilithium/mode{2,3,5}: the same
 * lattice, 32-byte tr and c~ (sign/dilithium/mode3/internal/params.go:5-18), key seed hashed without the K, L domain
 * bytes (internal/dilithium.go:191-193), mu = CRH(tr || msg) without a context prefix (mode3/dilithium.go:54-75) and
 * deterministic signing (no rnd, internal/dilithium.go:360-362).  For these modes contexts must be empty / NULL
 * (the reference fails with sign.ErrContextNotSupported) and rnd is ignored: the host-buffer entry points return
 * CIRCL_HIP_EPARAM when any context of the batch is non-empty; the device-resident ones (which cannot inspect the
 * offsets without synchronising) give ok[i] = 0 / an all-zero signature for such an item.
 *
 * ---- ML-DSA verify ----------------------------------------------------------------------
 * scheme.UnmarshalBinaryPublicKey(pk_i) + scheme.Verify(pk_i, msg_i, sig_i, &SignatureOpts{Context: ctx_i})
 * (sign/mldsa/mldsa65/dilithium.go:305-327 -> :115-132 -> internal/dilithium.go:273-332).
 * Messages / contexts are blobs with n+1 offsets; ctx_blob may be NULL (all contexts empty).
 * ok[i] = 1 valid, 0 invalid (bad encoding, norm bound, hint, hash mismatch or ctx > 255 bytes).
 */
int circl_hip_mldsa_verify(int param, const uint8_t *pk, const uint8_t *sig, const uint8_t *msg_blob,
                           const uint64_t *msg_off, const uint8_t *ctx_blob, const uint64_t *ctx_off,
                           uint8_t *ok, size_t n, int device);
/* ML-DSA.Verify_internal (message hashed without the context prefix): the reference's
 * unsafeVerifyInternal, sign/mldsa/mldsa65/dilithium.go:101-109, which its ACVP tests drive. */
int circl_hip_mldsa_verify_internal(int param, const uint8_t *pk, const uint8_t *sig,
                                    const uint8_t *msg_blob, const uint64_t *msg_off, uint8_t *ok,
                                    size_t n, int device);
size_t circl_hip_mldsa_workspace_size(int param, size_t n);
int circl_hip_mldsa_verify_dev(int param, const uint8_t *d_pk, const uint8_t *d_sig,
                               const uint8_t *d_msg_blob, const uint64_t *d_msg_off,
                               const uint8_t *d_ctx_blob, const uint64_t *d_ctx_off, uint8_t *d_ok,
                               size_t n, void *d_workspace, size_t workspace_bytes, void *stream);

/* Shared-key verification: all n signatures are checked under the ONE public key at `pk` -- n times
 * scheme.Verify(pk, msg_i, sig_i, opts_i) on one parsed key, where the reference caches A and tr in the PublicKey
 * object (sign/mldsa/mldsa65/internal/dilithium.go:114-126).  Same results as circl_hip_mldsa_verify on n copies of pk. */
int circl_hip_mldsa_verify_shared(int param, const uint8_t *pk, const uint8_t *sig, const uint8_t *msg_blob,
                                  const uint64_t *msg_off, const uint8_t *ctx_blob, const uint64_t *ctx_off,
                                  uint8_t *ok, size_t n, int device);
int circl_hip_mldsa_verify_shared_dev(int param, const uint8_t *d_pk, const uint8_t *d_sig,
                                      const uint8_t *d_msg_blob, const uint64_t *d_msg_off,
                                      const uint8_t *d_ctx_blob, const uint64_t *d_ctx_off, uint8_t *d_ok,
                                      size_t n, void *d_workspace, size_t workspace_bytes, void *stream);

/* Key-table verification: signature i is checked under row key_idx[i] of a table of nkeys public keys -- a verifier that
 * sees a few CA keys across a large batch.  tr and ExpandA (what PublicKey.Unpack caches per key,
 * sign/mldsa/mldsa65/internal/dilithium.go:114-126; benchmark note internal/dilithium_test.go:37-39) run once per TABLE
 * ENTRY.  Same results as circl_hip_mldsa_verify on the gathered rows.  The _dev variant needs
 * circl_hip_mldsa_keyed_workspace_size(param, n, nkeys) bytes and bounds d_key_idx to the table (>= nkeys: the last entry). */
int circl_hip_mldsa_verify_keyed(int param, const uint8_t *pk_table, size_t nkeys, const uint32_t *key_idx,
                                 const uint8_t *sig, const uint8_t *msg_blob, const uint64_t *msg_off,
                                 const uint8_t *ctx_blob, const uint64_t *ctx_off, uint8_t *ok, size_t n, int device);
size_t circl_hip_mldsa_keyed_workspace_size(int param, size_t n, size_t nkeys);
int circl_hip_mldsa_verify_keyed_dev(int param, const uint8_t *d_pk_table, size_t nkeys, const uint32_t *d_key_idx,
                                     const uint8_t *d_sig, const uint8_t *d_msg_blob, const uint64_t *d_msg_off,
                                     const uint8_t *d_ctx_blob, const uint64_t *d_ctx_off, uint8_t *d_ok, size_t n,
                                     void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- ML-DSA key generation ----------------------------------------------------------------
 * scheme.DeriveKey(seed_i), seed 32 bytes (sign/mldsa/mldsa65/dilithium.go:272-281 ->
 * internal/dilithium.go:181-267 NewKeyFromSeed); keys in MarshalBinary form.  The _dev variant
 * needs circl_hip_mldsa_workspace_size(param, n) bytes of workspace. */
int circl_hip_mldsa_keygen(int param, const uint8_t *seed32, uint8_t *pk, uint8_t *sk, size_t n,
                           int device);
int circl_hip_mldsa_keygen_dev(int param, const uint8_t *d_seed32, uint8_t *d_pk, uint8_t *d_sk,
                               size_t n, void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- ML-DSA signing ----------------------------------------------------
 * scheme.UnmarshalBinaryPrivateKey(sk_i) + scheme.Sign(sk_i, msg_i, &SignatureOpts{Context: ctx_i})
 * (sign/mldsa/mldsa65/dilithium.go:283-303 -> :56-88 SignTo -> internal/dilithium.go:340-470).
 * rnd[n][32] is the per-signature randomness the Go wrapper draws from crypto/rand when
 * `randomized` is set; rnd == NULL means deterministic signing (32 zero bytes).  A context longer
 * than 255 bytes makes the host-buffer call return CIRCL_HIP_EPARAM (sign.ErrContextTooLong).
 * circl_hip_mldsa_sign_internal is ML-DSA.Sign_internal (unsafeSignInternal, dilithium.go:90-99).
 * The _dev variant needs circl_hip_mldsa_sign_workspace_size(param, n) bytes (about 60 KB per item for
 * ML-DSA-65: expanded matrix and NTT-domain secrets per item); d_rnd must not be NULL.  An item whose context is
 * longer than 255 bytes gets an ALL-ZERO signature from the _dev variants (never one over a truncated length).
 * The workspace holds key-equivalent intermediates while the call runs; its secret regions are zeroed before the
 * call's work completes.  Like every other _dev call the signer is ASYNCHRONOUS: the rejection loop runs as rounds
 * over the list of unsigned items whose length lives in device memory; the host enqueues a fixed schedule of rounds
 * (sized so that the chance of an item surviving it is below 2^-40) followed by a persistent kernel that finishes
 * whatever is left, and never reads anything back, so nothing synchronises `stream`. */
int circl_hip_mldsa_sign(int param, const uint8_t *sk, const uint8_t *msg_blob, const uint64_t *msg_off,
                         const uint8_t *ctx_blob, const uint64_t *ctx_off, const uint8_t *rnd, uint8_t *sig,
                         size_t n, int device);
int circl_hip_mldsa_sign_internal(int param, const uint8_t *sk, const uint8_t *msg_blob,
                                  const uint64_t *msg_off, const uint8_t *rnd, uint8_t *sig, size_t n,
                                  int device);
/* Shared-key signing: all n messages are signed with the ONE private key at `sk` -- n times scheme.Sign(sk, msg_i, opts_i)
 * on one parsed key, where the reference caches A and the NTT-domain secrets in the PrivateKey
 * (sign/mldsa/mldsa65/internal/dilithium.go:149-179).  Same signatures as circl_hip_mldsa_sign on n copies of sk. */
int circl_hip_mldsa_sign_shared(int param, const uint8_t *sk, const uint8_t *msg_blob, const uint64_t *msg_off,
                                const uint8_t *ctx_blob, const uint64_t *ctx_off, const uint8_t *rnd, uint8_t *sig,
                                size_t n, int device);
int circl_hip_mldsa_sign_shared_dev(int param, const uint8_t *d_sk, const uint8_t *d_msg_blob,
                                    const uint64_t *d_msg_off, const uint8_t *d_ctx_blob, const uint64_t *d_ctx_off,
                                    const uint8_t *d_rnd, int internal, uint8_t *d_sig, size_t n, void *d_workspace,
                                    size_t workspace_bytes, void *stream);
size_t circl_hip_mldsa_sign_workspace_size(int param, size_t n);
int circl_hip_mldsa_sign_dev(int param, const uint8_t *d_sk, const uint8_t *d_msg_blob,
                             const uint64_t *d_msg_off, const uint8_t *d_ctx_blob, const uint64_t *d_ctx_off,
                             const uint8_t *d_rnd, int internal, uint8_t *d_sig, size_t n, void *d_workspace,
                             size_t workspace_bytes, void *stream);

/* ---- primitives (host buffers), mirroring the reference's unit-tested building blocks ----
 * circl_hip_keccak_f1600 : internal/sha3/keccakf.go:12 KeccakF1600 / simd/keccakf1600 StateX4.Permute
 *                          on n states of 25 little-endian uint64 words each; rounds = 24 or 12.
 * circl_hip_kyber_ntt    : pke/kyber/internal/common Poly.NTT (inverse=0) / Poly.InvNTT (1) on n
 *                          polynomials int16[256] in standard order.  Outputs are normalised to
 *                          [0,q) (the reference compares inverse transforms after Normalize,
 *                          ntt_test.go:64-81).
 * circl_hip_kyber_mulhat : Poly.MulHat, out[i] = a[i] (*) b[i], normalised.
 * circl_hip_dilithium_ntt: sign/internal/dilithium Poly.NTT / InvNTT on n polynomials uint32[256],
 *                          outputs normalised to [0,q).
 * circl_hip_shake        : n independent SHAKE128 (rate=168) / SHAKE256 (136) / SHA3-256 (136, ds 6)
 *                          / SHA3-512 (72, ds 6) computations over equal-length inputs
 *                          (internal/sha3 State.Write/Read).
 */
int circl_hip_keccak_f1600(uint64_t *states, size_t n, int rounds, int device);
/* the same 24-round permutation through the wave-cooperative form (one state per wavefront, lanes exchange through LDS)
 * that the ML-DSA kernels use on a rare serial path; exported so that the parity tests can pin it */
int circl_hip_keccak_f1600_coop(uint64_t *states, size_t n, int device);
/* the same through the two-lanes-per-state form (low halves on the even lane, high halves on the odd one, DPP exchange for
 * the rotations) that the small- and medium-batch hashing paths use; exported so that the parity tests can pin it */
int circl_hip_keccak_f1600_split(uint64_t *states, size_t n, int device);
/* sign/mldsa/mldsa65/internal/sample.go:299-339 PolyDeriveUniformBall: n challenge seeds c~ (32 / 48 / 64 bytes for
 * ML-DSA-44 / 65 / 87, 32 for the round-3 modes) -> n polynomials uint32[256] with tau coefficients in {1, q-1}.
 * sequential != 0 runs the reference-order byte scan (otherwise the fallback of the block-parallel form). */
int circl_hip_mldsa_sample_in_ball(int param, const uint8_t *ctilde, uint32_t *polys, size_t n, int sequential,
                                   int device);
int circl_hip_kyber_ntt(int16_t *polys, size_t n, int inverse, int device);
int circl_hip_kyber_mulhat(int16_t *out, const int16_t *a, const int16_t *b, size_t n, int device);

/* Lane-local arithmetic of the device code, elementwise over uint32 arrays (parity tests: the reference checks these
 * functions over their whole domains -- pke/kyber/internal/common/poly_test.go:351-378 compress = exact rounding,
 * sign/mldsa/mldsa65/internal/rounding_test.go:14-67 decompose / makeHint / useHint, field_test.go Montgomery / Barrett --
 * and the GPU instantiation uses different instructions than the host one).  out1 may be NULL; b may be NULL when unused. */
#define CIRCL_HIP_LANE_KYBER_COMPRESS 1    /* arg = d in {4,5,10,11}: out0 = round(a 2^d / q) mod 2^d for ANY representative a < 4q (poly.go:248-332) */
#define CIRCL_HIP_LANE_KYBER_DECOMPRESS 2  /* arg = d in {1,4,5,10,11}: out0 = round(a q / 2^d) (poly.go:170-243) */
#define CIRCL_HIP_LANE_KYBER_MSG_BIT 3     /* out0 = message bit of a in [0,q) (poly.go:150-165) */
#define CIRCL_HIP_LANE_KYBER_MULC 4        /* out0 = a b mod q in [0,q) for a < 2^32/q, via the R = 2^32 constant product (field.go:4-32 replaced) */
#define CIRCL_HIP_LANE_KYBER_REDUCE32 5    /* out0 = -a 2^-32 mod q in [0,q) for any 32-bit a */
#define CIRCL_HIP_LANE_KYBER_NORMALIZE 6   /* a = int16 in the low half: out0 = Normalize (poly.go:35-39), out1 = barrettReduce (field.go:45-64) */
#define CIRCL_HIP_LANE_KYBER_CBD2_WORD 7   /* out0 = the eight biased eta = 2 samples of the PRF word a, one per nibble (sample.go:67-95) */
#define CIRCL_HIP_LANE_KYBER_DOT2 8        /* out0 = lo16(a) lo16(b) + hi16(a) hi16(b) + arg (signed 16-bit halves): MulHat's multiply-accumulate */
#define CIRCL_HIP_LANE_DIL_DECOMPOSE 9     /* arg = gamma2 (95232 | 261888): out0 = a0 + q, out1 = a1 (rounding.go:13-43) */
#define CIRCL_HIP_LANE_DIL_USE_HINT 10     /* arg = gamma2, b = hint: out0 = useHint(a, b) (rounding.go:72-81) */
#define CIRCL_HIP_LANE_DIL_MAKE_HINT 11    /* arg = gamma2, a = z0, b = r1: out0 = makeHint (rounding.go:56-70) */
#define CIRCL_HIP_LANE_DIL_POWER2ROUND 12  /* out0 = a0 + q, out1 = a1 (sign/internal/dilithium/field.go:35-52) */
#define CIRCL_HIP_LANE_DIL_MONT32 13       /* out0 = a b 2^-32 mod q in (0, 2q) for a b < 2^32 q (field.go:20-24) */
#define CIRCL_HIP_LANE_DIL_MONT64 14       /* the same reduction of the 64-bit value b 2^32 + a < 2^32 q */
#define CIRCL_HIP_LANE_DIL_NORMALIZE 15    /* out0 = a mod q for any 32-bit a, out1 = the partial reduction fold(a) < 2^24 (field.go:5-13, :27-31) */
#define CIRCL_HIP_LANE_DIL_EXCEEDS 16      /* b = bound: out0 = 1 iff the centred |a| >= bound, a in [0,q) (poly.go:51-71) */
#define CIRCL_HIP_LANE_OP_COUNT 17
int circl_hip_lane_op(int op, int arg, const uint32_t *a, const uint32_t *b, uint32_t *out0, uint32_t *out1, size_t n, int device);

/* The samplers of the fused kernels with caller-chosen arguments (parity tests: the reference's fixed vectors use arguments the
 * fused kernels never do -- pke/kyber/internal/common/sample_test.go:23-138, sign/mldsa/mldsa65/internal/sample_test.go:12-63).
 * circl_hip_kyber_sample_uniform: Poly.DeriveUniform(seed_i, x_i, y_i) (sample.go:192-236), xy = n pairs of bytes ->
 *   polys[n][256] int16 in coefficient order, values in [0,q).
 * circl_hip_kyber_sample_cbd: Poly.DeriveNoise(seed_i, nonce, eta) for every nonce 0..63 (sample.go:17-95) ->
 *   polys[n][64][256] int16, centred values in [-eta, eta]; eta in {2, 3}.
 * circl_hip_mldsa_sample_uniform: PolyDeriveUniform(seed_i, nonce_i) (sign/mldsa/mldsa65/internal/sample.go:92-123) ->
 *   polys[n][256] uint32 in [0,q). */
int circl_hip_kyber_sample_uniform(const uint8_t *seed32, const uint8_t *xy, int16_t *polys, size_t n, int device);
int circl_hip_kyber_sample_cbd(int eta, const uint8_t *seed32, int16_t *polys, size_t n, int device);
int circl_hip_mldsa_sample_uniform(const uint8_t *seed32, const uint16_t *nonce, uint32_t *polys, size_t n, int device);
int circl_hip_dilithium_ntt(uint32_t *polys, size_t n, int inverse, int device);
int circl_hip_shake(int rate, int ds, const uint8_t *in, size_t inlen, uint8_t *out, size_t outlen,
                    size_t n, int device);
/* Batched XOF service (xof/xof.go, internal/sha3/shake.go:56-100): n independent
 * sponges over variable-length messages (blob + n+1 offsets), `rounds` = 24 (SHA3 / SHAKE) or 12
 * (TurboSHAKE128/256 with domain byte `ds` in 0x01..0x7f), every output `outlen` bytes. */
int circl_hip_xof(int rate, int ds, int rounds, const uint8_t *in_blob, const uint64_t *in_off,
                  uint8_t *out, size_t outlen, size_t n, int device);
/* KangarooTwelve draft -10, n independent computations: xof/k12/k12.go Draft10Sum(hash, msg_i, ctx_i)
 * (and xof.New(xof.K12D10) for an empty context, xof/xof.go:61-64).  Messages and contexts are blobs with
 * n+1 offsets; ctx_blob may be NULL (all contexts empty); every output is `outlen` bytes.  Leaves and final
 * nodes run as TurboSHAKE128 batches on the device. */
int circl_hip_k12(const uint8_t *msg_blob, const uint64_t *msg_off, const uint8_t *ctx_blob,
                  const uint64_t *ctx_off, uint8_t *out, size_t outlen, size_t n, int device);

/* ---- X25519 (the Diffie-Hellman half of X25519MLKEM768 and X-Wing) -------
 * Replaces dh/x25519: Shared(shared, secret, public) (key.go:41-47) with point != NULL, KeyGen(public, secret)
 * (key.go:34-36) with point == NULL (base point u = 9).  scalar, point, out are n rows of 32 bytes; the scalar is
 * clamped and bit 255 of the point is ignored, as the reference does.  ok[i] = 0 where Shared returns false (the point,
 * reduced mod 2^255 - 19, is one of the five low-order u-coordinates of curve.go:71-96; out[i] is then all zero),
 * 1 otherwise; ok may be NULL.  One Montgomery ladder per lane; device pointers 4-byte aligned. */
int circl_hip_x25519(const uint8_t *scalar, const uint8_t *point, uint8_t *out, uint8_t *ok, size_t n, int device);
int circl_hip_x25519_dev(const uint8_t *d_scalar, const uint8_t *d_point, uint8_t *d_out, uint8_t *d_ok, size_t n, void *stream);

/* ---- Ed25519 (sign/ed25519, pure Ed25519 of RFC 8032 5.1) -------------------------------------------------------
 * One key / signature per item, each item with its own key; messages are ragged: item i's message is
 * msg_blob[msg_off[i] .. msg_off[i+1]) (n + 1 offsets; msg_blob may be NULL when every message is empty).
 * circl_hip_ed25519_keygen: NewKeyFromSeed(seed_i) (ed25519.go:206-223).  pk[i] (32) = A = enc([s]B) with
 *   s = clamp(SHA-512(seed)[0..32)); sk[i] (64) = seed (32) || A (32), the reference's PrivateKey.  pk or sk may be NULL.
 * circl_hip_ed25519_sign: Sign(sk_i, msg_i) (ed25519.go:225-284 signAll, no context, no pre-hash).  sig[i] (64) = R (32) ||
 *   S (32, little-endian, below L): r = SHA-512(prefix || M) mod L with prefix = SHA-512(seed)[32..64), R = enc([r]B),
 *   k = SHA-512(R || sk[32..64) || M) mod L, S = r + k s mod L.  The second half of sk is hashed AS STORED: it is never
 *   recomputed from the seed nor checked against it, as in the reference.
 * circl_hip_ed25519_verify: Verify(pk_i, msg_i, sig_i) (ed25519.go:329-366).  ok[i] = 1 iff S < L, pk decodes (y < p, x
 *   exists, not x = 0 with the sign bit set: point.go:54-87) and enc([S]B - [k]A) equals the 32 bytes of R, k = SHA-512(R ||
 *   pk || M) mod L -- the cofactorless check, item by item (no batch shortcut: every ok[i] is the reference's verdict).  The
 *   ABI takes 64-byte signatures; a signature of any other length is the caller's to reject (the reference returns false).
 * The scheme has no context (SupportsContext() == false).
 * _dev forms: device pointers (rows 4-byte aligned, msg_off 8-byte aligned), any stream.  Verification needs
 *   circl_hip_ed25519_workspace_size(n) bytes of workspace (public multiples of the keys); key generation and signing keep
 *   their secrets (seed, s, prefix, r) in registers and leave the workspace untouched (it may be NULL).  The host forms
 *   wipe the device staging of seeds and private keys. */
size_t circl_hip_ed25519_workspace_size(size_t n);
int circl_hip_ed25519_keygen(const uint8_t *seed32, uint8_t *pk32, uint8_t *sk64, size_t n, int device);
int circl_hip_ed25519_sign(const uint8_t *sk64, const uint8_t *msg_blob, const uint64_t *msg_off, uint8_t *sig64, size_t n, int device);
int circl_hip_ed25519_verify(const uint8_t *pk32, const uint8_t *sig64, const uint8_t *msg_blob, const uint64_t *msg_off, uint8_t *ok,
                             size_t n, int device);
int circl_hip_ed25519_keygen_dev(const uint8_t *d_seed32, uint8_t *d_pk32, uint8_t *d_sk64, size_t n, void *d_workspace,
                                 size_t workspace_bytes, void *stream);
int circl_hip_ed25519_sign_dev(const uint8_t *d_sk64, const uint8_t *d_msg_blob, const uint64_t *d_msg_off, uint8_t *d_sig64, size_t n,
                               void *d_workspace, size_t workspace_bytes, void *stream);
int circl_hip_ed25519_verify_dev(const uint8_t *d_pk32, const uint8_t *d_sig64, const uint8_t *d_msg_blob, const uint64_t *d_msg_off,
                                 uint8_t *d_ok, size_t n, void *d_workspace, size_t workspace_bytes, void *stream);
/* FIPS 180-4 SHA-512 of every message (crypto/sha512.Sum512): out64[i] = the 64-byte digest of item i. */
int circl_hip_sha512(const uint8_t *msg_blob, const uint64_t *msg_off, uint8_t *out64, size_t n, int device);

/* ---- Ed25519-Dilithium2 (sign/eddilithium2/eddilithium.go): round-3 Dilithium2 (sign/dilithium/mode2) next to Ed25519 ----
 * circl_hip_eddilithium2_keygen: NewKeyFromSeed(seed_i): SHAKE256(seed) -> 32 bytes for mode2, then 32 for Ed25519.
 *   pk[i] (1344) = mode2 pk (1312) || Ed25519 pk (32); sk[i] (2560) = mode2 sk (2528) || the Ed25519 SEED (32).
 * circl_hip_eddilithium2_sign: SignTo (:150-162): sig[i] (2484) = the deterministic mode2 signature (2420) || the Ed25519
 *   signature (64) of the same message, the Ed25519 key re-derived from the seed in sk (Unpack, :127-132).
 * circl_hip_eddilithium2_verify: Verify (:166-171): ok[i] = 1 iff both halves verify.  A signature of any other length than
 *   2484 bytes is false in the reference; the ABI takes 2484-byte rows, so that check is the caller's.
 * No context (SupportsContext() == false).  Both halves run on the device, on one stream per chunk, with no host round trip
 * between them; the device staging and workspace of keygen and sign (both private keys) are zeroed after every chunk. */
int circl_hip_eddilithium2_keygen(const uint8_t *seed32, uint8_t *pk, uint8_t *sk, size_t n, int device);
int circl_hip_eddilithium2_sign(const uint8_t *sk, const uint8_t *msg_blob, const uint64_t *msg_off, uint8_t *sig, size_t n, int device);
int circl_hip_eddilithium2_verify(const uint8_t *pk, const uint8_t *sig, const uint8_t *msg_blob, const uint64_t *msg_off, uint8_t *ok,
                                  size_t n, int device);

/* ---- X448 (dh/x448, RFC 7748) -----------------------------------------------------------------------------------------
 * Shared(shared, secret, public) (key.go:41-46) with point != NULL, KeyGen(public, secret) (key.go:33-35) with point == NULL
 * (base point u = 5).  scalar, point, out are n rows of 56 bytes; the scalar is clamped (k[0] &= 252, k[55] |= 128,
 * key.go:15-20).  ok[i] = 0 where Shared returns false: the point, reduced mod p = 2^448 - 2^224 - 1, is 0, 1 or p - 1
 * (lowOrderPoints, curve.go:76; out[i] is then all zero), 1 otherwise; ok may be NULL.  One Montgomery ladder per lane for Shared;
 * KeyGen is the fixed-base comb of Ed448 followed by RFC 7748's isogeny u = y^2 / x^2 or, with CIRCL_HIP_X448_KEYGEN=ladder in
 * the environment, the same ladder from u = 5 (the reference's KeyGen is a Joye ladder over table.go); the same bytes either way.  Device pointers 4-byte aligned. */
int circl_hip_x448(const uint8_t *scalar, const uint8_t *point, uint8_t *out, uint8_t *ok, size_t n, int device);
int circl_hip_x448_dev(const uint8_t *d_scalar, const uint8_t *d_point, uint8_t *d_out, uint8_t *d_ok, size_t n, void *stream);

/* ---- Ed448 (sign/ed448, pure Ed448 of RFC 8032 5.2, with a context) -----------------------------------------------------
 * One key / signature per item, each item with its own key, message and context; messages and contexts are ragged: item i's
 * message is msg_blob[msg_off[i] .. msg_off[i+1]) and its context ctx_blob[ctx_off[i] .. ctx_off[i+1]) (n + 1 offsets each).
 * ctx_blob == NULL: every context is empty (ctx_off is then ignored), as in circl_hip_k12 and the ML-DSA calls.
 * circl_hip_ed448_keygen: NewKeyFromSeed(seed_i) (ed448.go).  pk[i] (57) = A = enc([s]B) with s = SHAKE256(seed, 114)[0..57)
 *   clamped (h[0] &= 0xFC, h[55] |= 0x80, h[56] = 0); sk[i] (114) = seed (57) || A (57), the reference's PrivateKey.  pk or sk
 *   may be NULL.
 * circl_hip_ed448_sign: Sign(sk_i, msg_i, ctx_i) (ed448.go signAll, no pre-hash).  sig[i] (114) = R (57) || S (57, little-endian,
 *   below l, byte 56 zero): dom4 = "SigEd448" || 0x00 || len(ctx) || ctx, r = SHAKE256(dom4 || prefix || M, 114) mod l with
 *   prefix = SHAKE256(seed, 114)[57..114), R = enc([r]B), k = SHAKE256(dom4 || R || sk[57..114) || M, 114) mod l, S = r + k s mod
 *   l.  The second half of sk is hashed AS STORED, as in the reference.  A context over 255 bytes: CIRCL_HIP_EPARAM before any
 *   launch (the reference panics); the _dev form, which cannot see the offsets, writes an all-zero signature for that item.
 * circl_hip_ed448_verify: Verify(pk_i, msg_i, sig_i, ctx_i) (ed448.go:294-339).  ok[i] = 1 iff the context is at most 255 bytes,
 *   S < l with byte 56 zero (isLessThanOrder), pk decodes (ecc/goldilocks point.go:43-80: low seven bits of byte 56 zero, y < p,
 *   x exists, not x = 0 with the sign bit set) and enc(Q) equals the 57 bytes of R, where Q is what goldilocks.Curve.
 *   CombinedMult(S, k, -A) returns (curve.go:80-90): 4 ([S/4 mod l]B + [k/4 mod l](-A)), k = SHAKE256(dom4 || R || pk || M, 114)
 *   mod l.  That is [S]B - [k]A with A's 4-torsion component dropped: neither the cofactorless nor RFC 8032's cofactored check;
 *   item by item, every ok[i] is the reference's verdict.  The ABI takes 57-byte keys and 114-byte signatures; other lengths are
 *   the caller's to reject (the reference returns false).  SupportsContext() == true; Ed448ph is not provided.
 * _dev forms: device pointers, any stream; the 57- and 114-byte rows need no alignment (they are READ as the aligned 4-byte
 *   words that hold them, so up to 3 bytes before and after a row's buffer are touched and masked off; writes are exact), offsets
 *   8-byte aligned.  Verification
 *   needs circl_hip_ed448_workspace_size(n) bytes of workspace (public multiples of the keys, 4-byte aligned); key generation
 *   and signing keep their secrets (seed, s, prefix, r) in registers and leave the workspace untouched (it may be NULL).  The
 *   host forms wipe the device staging of seeds and private keys. */
size_t circl_hip_ed448_workspace_size(size_t n);
int circl_hip_ed448_keygen(const uint8_t *seed57, uint8_t *pk57, uint8_t *sk114, size_t n, int device);
int circl_hip_ed448_sign(const uint8_t *sk114, const uint8_t *msg_blob, const uint64_t *msg_off, const uint8_t *ctx_blob,
                         const uint64_t *ctx_off, uint8_t *sig114, size_t n, int device);
int circl_hip_ed448_verify(const uint8_t *pk57, const uint8_t *sig114, const uint8_t *msg_blob, const uint64_t *msg_off,
                           const uint8_t *ctx_blob, const uint64_t *ctx_off, uint8_t *ok, size_t n, int device);
int circl_hip_ed448_keygen_dev(const uint8_t *d_seed57, uint8_t *d_pk57, uint8_t *d_sk114, size_t n, void *d_workspace,
                               size_t workspace_bytes, void *stream);
int circl_hip_ed448_sign_dev(const uint8_t *d_sk114, const uint8_t *d_msg_blob, const uint64_t *d_msg_off, const uint8_t *d_ctx_blob,
                             const uint64_t *d_ctx_off, uint8_t *d_sig114, size_t n, void *d_workspace, size_t workspace_bytes,
                             void *stream);
int circl_hip_ed448_verify_dev(const uint8_t *d_pk57, const uint8_t *d_sig114, const uint8_t *d_msg_blob, const uint64_t *d_msg_off,
                               const uint8_t *d_ctx_blob, const uint64_t *d_ctx_off, uint8_t *d_ok, size_t n, void *d_workspace,
                               size_t workspace_bytes, void *stream);

/* ---- Ed448-Dilithium3 (sign/eddilithium3/eddilithium.go): round-3 Dilithium3 (sign/dilithium/mode3) next to Ed448 -------
 * circl_hip_eddilithium3_keygen: NewKeyFromSeed(seed_i) (57 bytes): SHAKE256(seed) -> 32 bytes for mode3, then 57 for Ed448.
 *   pk[i] (2009) = mode3 pk (1952) || Ed448 pk (57); sk[i] (4057) = mode3 sk (4000) || the Ed448 SEED (57).
 * circl_hip_eddilithium3_sign: SignTo: sig[i] (3407) = the deterministic mode3 signature (3293) || the Ed448 signature (114) of
 *   the same message under the empty context, the Ed448 key re-derived from the seed in sk (Unpack).
 * circl_hip_eddilithium3_verify: Verify: ok[i] = 1 iff both halves verify.  A signature of any other length than 3407 bytes is
 *   false in the reference; the ABI takes 3407-byte rows, so that check is the caller's.
 * No context (SupportsContext() == false).  Both halves run on the device, on one stream per chunk, with no host round trip
 * between them; the device staging and workspace of keygen and sign (both private keys) are zeroed after every chunk. */
int circl_hip_eddilithium3_keygen(const uint8_t *seed57, uint8_t *pk, uint8_t *sk, size_t n, int device);
int circl_hip_eddilithium3_sign(const uint8_t *sk, const uint8_t *msg_blob, const uint64_t *msg_off, uint8_t *sig, size_t n, int device);
int circl_hip_eddilithium3_verify(const uint8_t *pk, const uint8_t *sig, const uint8_t *msg_blob, const uint64_t *msg_off, uint8_t *ok,
                                  size_t n, int device);

/* ---- FrodoKEM-640-SHAKE (kem/frodo/frodo640shake): N = 640, nbar = 8, q = 2^15, B = 2 ------------------------------------
 * circl_hip_frodo640shake_keygen: newKeyFromSeed(seed_i) (48 bytes = s || seedSE || z): seedA = SHAKE128(z)[:16],
 *   S^T || E sampled from SHAKE128(0x5F || seedSE), B = A S + E; pk[i] (9616) = seedA || pack15(B); sk[i] (19888) = s || pk ||
 *   S^T as 16-bit little-endian words || SHAKE128(pk)[:16].
 * circl_hip_frodo640shake_encaps: EncapsulateTo(pk_i, seed_i) (16 bytes = mu): ct[i] (9720) = pack15(S'A + E') ||
 *   pack15(S'B + E'' + encode(mu)), ss[i] (16) = SHAKE128(ct || k)[:16].
 * circl_hip_frodo640shake_decaps: DecapsulateTo: mu' from C - B'S, re-encryption to the pk stored in sk with the hpk stored in
 *   sk, ss[i] = SHAKE128(ct || k') when both halves match and SHAKE128(ct || s) otherwise, chosen without a branch.
 * The keys are taken as stored, as the reference takes them: A's words are raw 16-bit SHAKE output, arithmetic is mod 2^16 with
 *   the 15-bit mask only where the reference has it, the S words of a private key are arbitrary uint16, and neither the stored
 *   hpk nor the key's own consistency is checked.  The ABI takes rows of the six sizes below; other lengths are the caller's to
 *   reject (the reference panics or returns kem.ErrCiphertextSize).
 * A (800 KB per item) is never stored: its 640 SHAKE128 rows are squeezed and consumed inside the matrix kernel.
 * _dev forms: device pointers, any stream.  The key, ciphertext, seed and secret rows need NO alignment: they are read as the
 *   aligned 4-byte words that hold them (up to 3 bytes before and after a row's buffer are touched and masked off) and written
 *   byte by byte.  The workspace (S', E', E'', mu', k', the re-encryption -- all secret) is
 *   circl_hip_frodo640shake_workspace_size(n) bytes, 16-byte aligned, the same for the three calls and monotone in n; every
 *   call zeroes it on the stream behind its kernels.  The host forms also wipe the device staging of every chunk.
 * Errors: CIRCL_HIP_ENODEV without a device, CIRCL_HIP_EPARAM for a NULL pointer, CIRCL_HIP_EWORKSPACE for a short or misaligned
 *   workspace; n = 0 is CIRCL_HIP_OK. */
#define CIRCL_HIP_FRODO640SHAKE_PK_BYTES 9616
#define CIRCL_HIP_FRODO640SHAKE_SK_BYTES 19888
#define CIRCL_HIP_FRODO640SHAKE_CT_BYTES 9720
#define CIRCL_HIP_FRODO640SHAKE_SS_BYTES 16
#define CIRCL_HIP_FRODO640SHAKE_KEYSEED_BYTES 48
#define CIRCL_HIP_FRODO640SHAKE_ENCSEED_BYTES 16
size_t circl_hip_frodo640shake_workspace_size(size_t n);
int circl_hip_frodo640shake_keygen(const uint8_t *seed48, uint8_t *pk, uint8_t *sk, size_t n, int device);
int circl_hip_frodo640shake_encaps(const uint8_t *pk, const uint8_t *seed16, uint8_t *ct, uint8_t *ss, size_t n, int device);
int circl_hip_frodo640shake_decaps(const uint8_t *sk, const uint8_t *ct, uint8_t *ss, size_t n, int device);
int circl_hip_frodo640shake_keygen_dev(const uint8_t *d_seed48, uint8_t *d_pk, uint8_t *d_sk, size_t n, void *d_workspace,
                                       size_t workspace_bytes, void *stream);
int circl_hip_frodo640shake_encaps_dev(const uint8_t *d_pk, const uint8_t *d_seed16, uint8_t *d_ct, uint8_t *d_ss, size_t n,
                                       void *d_workspace, size_t workspace_bytes, void *stream);
int circl_hip_frodo640shake_decaps_dev(const uint8_t *d_sk, const uint8_t *d_ct, uint8_t *d_ss, size_t n, void *d_workspace,
                                       size_t workspace_bytes, void *stream);

/* ---- hybrid KEMs around ML-KEM-768, composed on the device -------------------------------
 * scheme = CIRCL_HIP_HYBRID_XWING: kem/xwing/xwing.go -- DeriveKeyPairPacked (:98-144), EncapsulateTo (:223-265),
 *   DecapsulateTo (:270-299), combiner (:53-71).  seed 32, eseed 64 (seedm || ekx), pk 1216 (ek || pk_X), sk 32 (the
 *   seed), ct 1120 (ct_M || ct_X), ss 32.  status[i] = 1 (kem.ErrPubKey) when the ML-KEM half of pk fails the
 *   encapsulation-key check (xwing.go:301-311); a low-order X25519 point is not an error (xwing.go:251-254).
 * scheme = CIRCL_HIP_HYBRID_X25519MLKEM768: kem/hybrid/hybrid.go (:236-323) with X25519 as a KEM (xkem.go:112-196).
 *   seed 64, eseed 32, pk 1216 (ek || pk_X), sk 2432 (dk || sk_X), ct 1120, ss 64 (ss_M || ss_X).  status[i] = 1
 *   (kem.ErrPubKey) for a non-canonical ek or a low-order X25519 point, 2 (kem.ErrPrivKey) for a private key failing its
 *   hash check; the item's outputs are then zero (the reference returns nil, err).
 * scheme = CIRCL_HIP_HYBRID_KYBER768_X25519 / _KYBER512_X25519: the same hybrid.go scheme with X25519 as the FIRST component
 *   and round-3 Kyber (kem/kyber) as the second: pk = pk_X || ek (1216 / 832), sk = sk_X || dk (2432 / 1664), ct = ct_X ||
 *   ct_K (1120 / 800), ss = ss_X || ss_K (64); seed 64 (SHAKE256 -> 32 for X25519, then 64 for Kyber), eseed 32.  Round-3
 *   Kyber has no per-item failure, so status is 1 only for a low-order X25519 point.
 * scheme = CIRCL_HIP_HYBRID_KYBER768_X448 / _KYBER1024_X448: the same with X448 as a KEM (xkem.go, 56-byte rows) as the first
 *   component and round-3 Kyber768 / Kyber1024 as the second: pk = pk_X || ek (1240 / 1624), sk = sk_X || dk (2456 / 3224),
 *   ct = ct_X || ct_K (1144 / 1624), ss = ss_X || ss_K (88); seed 64 (SHAKE256 -> 56 for X448, then 64 for Kyber), eseed 56
 *   (SHAKE256 -> 56 for X448, then 32 for Kyber).  status is 1 only where the X448 point, reduced mod p, is 0, 1 or p - 1
 *   (dh/x448/key.go:22-30).  These two have no key tables, no coalescing and no asynchronous queue: circl_hip_hybrid_keytable_new
 *   and circl_hip_queue_open return CIRCL_HIP_EPARAM for them.
 * The deterministic forms only (EncapsulateDeterministically / DeriveKeyPair): randomness stays with the caller.
 * The _dev forms zero the secret temporaries in the workspace (seeds, X25519 / X448 scalars, private keys, half secrets) before
 * they return control of the stream; the ML-KEM workspace behind them follows the rules of the ML-KEM entry points.
 * status may be NULL on the host forms.  The _dev forms need circl_hip_hybrid_workspace_size(scheme, n) bytes, 16-byte
 * aligned arrays, and a non-NULL d_status. */
#define CIRCL_HIP_HYBRID_XWING 1
#define CIRCL_HIP_HYBRID_X25519MLKEM768 2
#define CIRCL_HIP_HYBRID_KYBER768_X25519 3 /* hybrid.Kyber768X25519(): X25519 first, round-3 Kyber768 second (hybrid.go:77-81) */
#define CIRCL_HIP_HYBRID_KYBER512_X25519 4 /* hybrid.Kyber512X25519() (hybrid.go:71-75) */
#define CIRCL_HIP_HYBRID_KYBER768_X448 5   /* hybrid.Kyber768X448():  X448 first, round-3 Kyber768 second  (hybrid.go:83-87) */
#define CIRCL_HIP_HYBRID_KYBER1024_X448 6  /* hybrid.Kyber1024X448(): X448 first, round-3 Kyber1024 second (hybrid.go:89-93) */
size_t circl_hip_hybrid_seed_size(int scheme);
size_t circl_hip_hybrid_eseed_size(int scheme);
size_t circl_hip_hybrid_pk_size(int scheme);
size_t circl_hip_hybrid_sk_size(int scheme);
size_t circl_hip_hybrid_ct_size(int scheme);
size_t circl_hip_hybrid_ss_size(int scheme);
size_t circl_hip_hybrid_workspace_size(int scheme, size_t n);
int circl_hip_hybrid_keygen(int scheme, const uint8_t *seed, uint8_t *pk, uint8_t *sk, size_t n, int device);
int circl_hip_hybrid_encaps(int scheme, const uint8_t *pk, const uint8_t *eseed, uint8_t *ct, uint8_t *ss, uint8_t *status, size_t n, int device);
int circl_hip_hybrid_decaps(int scheme, const uint8_t *sk, const uint8_t *ct, uint8_t *ss, uint8_t *status, size_t n, int device);
int circl_hip_hybrid_keygen_dev(int scheme, const uint8_t *d_seed, uint8_t *d_pk, uint8_t *d_sk, size_t n, void *d_ws, size_t ws_bytes, void *stream);
int circl_hip_hybrid_encaps_dev(int scheme, const uint8_t *d_pk, const uint8_t *d_eseed, uint8_t *d_ct, uint8_t *d_ss, uint8_t *d_status, size_t n,
                                void *d_ws, size_t ws_bytes, void *stream);
int circl_hip_hybrid_decaps_dev(int scheme, const uint8_t *d_sk, const uint8_t *d_ct, uint8_t *d_ss, uint8_t *d_status, size_t n, void *d_ws,
                                size_t ws_bytes, void *stream);

/* Hybrid key tables that live across calls (scheme = CIRCL_HIP_HYBRID_XWING or _X25519MLKEM768): kem/xwing's PrivateKey keeps the
 * expanded ML-KEM-768 key, the X25519 scalar and its public point next to the 32-byte seed (xwing.go:20-25), its PublicKey the
 * parsed ML-KEM key; kem/hybrid's keys hold the component schemes' parsed keys (hybrid.go:101-114).  keys = nkeys packed public
 * (private_keys = 0) or private (1) keys of the scheme; an X-Wing private key (the seed) is expanded ONCE, on the device.  The table
 * holds an ML-KEM key table of the lattice halves (A^T, H(ek), hash verdicts -> key_status[nkeys] if not NULL) and the X25519
 * rows.  Item i uses entry key_idx[i] (NULL: entry 0).  Results are those of circl_hip_hybrid_encaps / _decaps on the gathered
 * keys.  The _dev forms need circl_hip_hybrid_workspace_size(scheme, n) bytes. */
int circl_hip_hybrid_keytable_new(int scheme, int private_keys, const uint8_t *keys, size_t nkeys, int device, uint8_t *key_status,
                                  circl_hip_keytable **out);
int circl_hip_hybrid_encaps_table(const circl_hip_keytable *table, const uint32_t *key_idx, const uint8_t *eseed, uint8_t *ct, uint8_t *ss,
                                  uint8_t *status, size_t n);
int circl_hip_hybrid_decaps_table(const circl_hip_keytable *table, const uint32_t *key_idx, const uint8_t *ct, uint8_t *ss, uint8_t *status,
                                  size_t n);
int circl_hip_hybrid_encaps_table_dev(const circl_hip_keytable *table, const uint32_t *d_key_idx, const uint8_t *d_eseed, uint8_t *d_ct,
                                      uint8_t *d_ss, uint8_t *d_status, size_t n, void *d_ws, size_t ws_bytes, void *stream);
int circl_hip_hybrid_decaps_table_dev(const circl_hip_keytable *table, const uint32_t *d_key_idx, const uint8_t *d_ct, uint8_t *d_ss,
                                      uint8_t *d_status, size_t n, void *d_ws, size_t ws_bytes, void *stream);

/* ---- HPKE DHKEM over X25519 and X448 (hpke/kembase.go, hpke/xkem.go; RFC 9180 section 4.1) ------------------------------
 * kem = CIRCL_HIP_HPKE_KEM_X25519_HKDF_SHA256 (0x20) or CIRCL_HIP_HPKE_KEM_X448_HKDF_SHA512 (0x21); any other value is
 * CIRCL_HIP_EPARAM.  Every key row (ikm, sk, pk, enc) is circl_hip_hpke_dhkem_key_size(kem) = 32 / 56 bytes, a shared secret
 * circl_hip_hpke_dhkem_ss_size(kem) = 32 / 64 bytes (kemBase.SharedKeySize = the hash size); both return 0 for an unknown kem.
 * One fused kernel per call and one item per lane: the scalar multiplications (the fixed-base comb for a public key, the
 * Montgomery ladder for a Diffie-Hellman output) and the HKDF between them run in one launch, without a workspace; the ephemeral
 * private key, the Diffie-Hellman outputs and the HKDF pseudorandom keys stay in the lane.
 *   derive_keypair: xKEM.DeriveKeyPair(ikm): sk = LabeledExpand(LabeledExtract("", "dkp_prk", ikm), "sk", "", Nsk), the raw Expand
 *     output (unclamped, as the reference stores it); pk = KeyGen(sk).
 *   encap:      EncapsulateDeterministically(pkR, ikmE) -> enc, ss.
 *   decap:      Decapsulate(skR, enc) -> ss.
 *   auth_encap: AuthEncapsulateDeterministically(pkR, skS, ikmE) -> enc, ss.
 *   auth_decap: AuthDecapsulate(skR, enc, pkS) -> ss.
 * The private key's own public key (pkR of decap / auth_decap, pkS of auth_encap) may be NULL: the kernel then computes it with
 * the comb (the reference caches Public()).  kemCtx is built from the public-key bytes exactly as given: X25519 ignores bit 255 of
 * a point in the ladder, but the bit still enters kemCtx (MarshalBinary returns the stored bytes).
 * ok[i] = 0 where a Shared of item i returns false (the low-order points circl_hip_x25519 / circl_hip_x448 flag); ss[i], and
 * enc[i] for the encapsulations, are then all zero (the reference returns nil, err).  ok may be NULL.
 * GenerateKeyPair (a random sk, pk = KeyGen(sk)) is circl_hip_x25519 / circl_hip_x448 with point == NULL on sk rows the caller
 * drew: there is no call of its own for it.
 * The host forms stage through the pipeline and zero the device staging of every chunk; the _dev forms want 4-byte aligned
 * pointers (CIRCL_HIP_EWORKSPACE otherwise).  n == 0 is CIRCL_HIP_OK. */
#define CIRCL_HIP_HPKE_KEM_X25519_HKDF_SHA256 0x20
#define CIRCL_HIP_HPKE_KEM_X448_HKDF_SHA512 0x21
size_t circl_hip_hpke_dhkem_key_size(int kem);
size_t circl_hip_hpke_dhkem_ss_size(int kem);
int circl_hip_hpke_dhkem_derive_keypair(int kem, const uint8_t *ikm, uint8_t *sk, uint8_t *pk, size_t n, int device);
int circl_hip_hpke_dhkem_encap(int kem, const uint8_t *pkR, const uint8_t *ikmE, uint8_t *enc, uint8_t *ss, uint8_t *ok, size_t n, int device);
int circl_hip_hpke_dhkem_decap(int kem, const uint8_t *skR, const uint8_t *pkR, const uint8_t *enc, uint8_t *ss, uint8_t *ok, size_t n, int device);
int circl_hip_hpke_dhkem_auth_encap(int kem, const uint8_t *pkR, const uint8_t *skS, const uint8_t *pkS, const uint8_t *ikmE, uint8_t *enc, uint8_t *ss,
                                    uint8_t *ok, size_t n, int device);
int circl_hip_hpke_dhkem_auth_decap(int kem, const uint8_t *skR, const uint8_t *pkR, const uint8_t *enc, const uint8_t *pkS, uint8_t *ss, uint8_t *ok,
                                    size_t n, int device);
int circl_hip_hpke_dhkem_derive_keypair_dev(int kem, const uint8_t *d_ikm, uint8_t *d_sk, uint8_t *d_pk, size_t n, void *stream);
int circl_hip_hpke_dhkem_encap_dev(int kem, const uint8_t *d_pkR, const uint8_t *d_ikmE, uint8_t *d_enc, uint8_t *d_ss, uint8_t *d_ok, size_t n,
                                   void *stream);
int circl_hip_hpke_dhkem_decap_dev(int kem, const uint8_t *d_skR, const uint8_t *d_pkR, const uint8_t *d_enc, uint8_t *d_ss, uint8_t *d_ok, size_t n,
                                   void *stream);
int circl_hip_hpke_dhkem_auth_encap_dev(int kem, const uint8_t *d_pkR, const uint8_t *d_skS, const uint8_t *d_pkS, const uint8_t *d_ikmE, uint8_t *d_enc,
                                        uint8_t *d_ss, uint8_t *d_ok, size_t n, void *stream);
int circl_hip_hpke_dhkem_auth_decap_dev(int kem, const uint8_t *d_skR, const uint8_t *d_pkR, const uint8_t *d_enc, const uint8_t *d_pkS, uint8_t *d_ss,
                                        uint8_t *d_ok, size_t n, void *stream);
/* FIPS 180-4 SHA-256 of every message (crypto/sha256.Sum256): out32[i] = the 32-byte digest of item i; the ragged layout of
 * circl_hip_sha512. */
int circl_hip_sha256(const uint8_t *msg_blob, const uint64_t *msg_off, uint8_t *out32, size_t n, int device);

/* ---- HPKE contexts: key schedule, ChaCha20-Poly1305 Seal / Open, Export (hpke/hpke.go, hpke/util.go, hpke/aead.go; RFC 9180
 * sections 5 and 6) ---------------------------------------------------------------------------------------------------------
 * A suite is (kem, kdf, aead): kem = 0x20 / 0x21 as above, kdf = CIRCL_HIP_HPKE_KDF_HKDF_SHA256 (1) or _SHA512 (3), any KDF with
 * any KEM, aead = CIRCL_HIP_HPKE_AEAD_CHACHA20POLY1305 (3) or CIRCL_HIP_HPKE_AEAD_EXPORT_ONLY (0xFFFF); mode = 0 base, 1 psk,
 * 2 auth, 3 auth_psk.  Every other code point (HKDF-SHA384, the AES-GCM AEADs, the P-curve and hybrid KEMs) and mode > 3 are
 * CIRCL_HIP_EPARAM, reported before a device is looked for, as is every breach of the rules below.
 * One item per lane, one launch per call, no workspace.  A setup runs the DHKEM operation and the key schedule in one kernel; the
 * shared secret stays in the lane.  Its result is a CONTEXT ROW of circl_hip_hpke_context_size(kdf) = 48 + Nh = 80 / 112 bytes
 * (0 for an unknown kdf): key[32] || base_nonce[12] || 0[4] || exporter_secret[Nh]; key and base_nonce are zero for export-only.
 * Context rows are secret and 4-byte aligned; Seal / Open / Export read them at ctx_stride bytes apart (a multiple of 4, at least
 * 48 for Seal / Open and the context size for Export).
 * Ragged arguments (info, psk, psk_id, aad, the exporter context, plaintexts) are a blob and n + 1 uint64_t offsets; a NULL blob
 * means that every item's input is empty (its offsets are then not read).  Item i's plaintext is pt_off[i + 1] - pt_off[i] bytes
 * at pt_blob[pt_off[i]]; its ciphertext (ct || tag) is 16 bytes longer at ct_blob[pt_off[i] + 16 i]: the one offset array
 * describes both sides.  The ciphertext blob of Open is required.
 *   setup_sender:   SetupBase/PSK/Auth/AuthPSK S with the ephemeral key derived from ikmE -> enc, ctx.  skS and pkS are NULL in
 *                   modes 0 and 1 and both required in modes 2 and 3.
 *   setup_receiver: SetupBase/PSK/Auth/AuthPSK R -> ctx.  pkR (the receiver's own public key) may be NULL; pkS is NULL in modes
 *                   0 and 1 and required in modes 2 and 3.
 *   psk / psk_id:   the blobs must be NULL in modes 0 and 2.  In modes 1 and 3 an item whose psk or psk_id is empty fails
 *                   (verifyPSKInputs); there is no minimum psk length, as in the reference.
 *   seal / open:    ChaCha20-Poly1305 under key and base_nonce XOR BE96(seq[i]) (seq == NULL: 0).  The caller owns the sequence
 *                   numbers.  Open verifies the tag before it decrypts.  aead must be CHACHA20POLY1305.
 *   export:         LabeledExpand(exporter_secret, "sec", exporter_context_i, L), 1 <= L <= 255 Nh, out = n rows of L bytes.
 *   *_single:       RFC 9180 section 6: setup and a Seal / Open at sequence number 0, or an Export, in ONE kernel; neither the
 *                   shared secret nor the context reaches memory.
 * ok[i] = 0 and every output row of item i all zero where the KEM fails (a low-order point), the psk rule fails or, for Open,
 * the tag does not verify.  ok may be NULL.  The host forms zero their staging; the _dev forms want 4-byte aligned rows and
 * 8-byte aligned offset and seq arrays (CIRCL_HIP_EWORKSPACE otherwise).  n == 0 is CIRCL_HIP_OK. */
#define CIRCL_HIP_HPKE_KDF_HKDF_SHA256 0x0001
#define CIRCL_HIP_HPKE_KDF_HKDF_SHA512 0x0003
#define CIRCL_HIP_HPKE_AEAD_CHACHA20POLY1305 0x0003
#define CIRCL_HIP_HPKE_AEAD_EXPORT_ONLY 0xFFFF
size_t circl_hip_hpke_context_size(int kdf);
#define CIRCL_HIP_HPKE_SENDER_                                                                                                                       \
    int kem, int kdf, int aead, int mode, const uint8_t *pkR, const uint8_t *ikmE, const uint8_t *skS, const uint8_t *pkS, const uint8_t *info_blob, \
        const uint64_t *info_off, const uint8_t *psk_blob, const uint64_t *psk_off, const uint8_t *psk_id_blob, const uint64_t *psk_id_off
#define CIRCL_HIP_HPKE_RECEIVER_                                                                                                                    \
    int kem, int kdf, int aead, int mode, const uint8_t *skR, const uint8_t *pkR, const uint8_t *enc, const uint8_t *pkS, const uint8_t *info_blob, \
        const uint64_t *info_off, const uint8_t *psk_blob, const uint64_t *psk_off, const uint8_t *psk_id_blob, const uint64_t *psk_id_off
#define CIRCL_HIP_HPKE_SEAL_ const uint8_t *pt_blob, const uint64_t *pt_off, const uint8_t *aad_blob, const uint64_t *aad_off
#define CIRCL_HIP_HPKE_OPEN_ const uint8_t *ct_blob, const uint64_t *pt_off, const uint8_t *aad_blob, const uint64_t *aad_off
#define CIRCL_HIP_HPKE_ROWS_ const uint8_t *ctx, size_t ctx_stride
int circl_hip_hpke_setup_sender(CIRCL_HIP_HPKE_SENDER_, uint8_t *enc, uint8_t *ctx, uint8_t *ok, size_t n, int device);
int circl_hip_hpke_setup_receiver(CIRCL_HIP_HPKE_RECEIVER_, uint8_t *ctx, uint8_t *ok, size_t n, int device);
int circl_hip_hpke_seal(int aead, CIRCL_HIP_HPKE_ROWS_, const uint64_t *seq, CIRCL_HIP_HPKE_SEAL_, uint8_t *ct_blob, size_t n, int device);
int circl_hip_hpke_open(int aead, CIRCL_HIP_HPKE_ROWS_, const uint64_t *seq, CIRCL_HIP_HPKE_OPEN_, uint8_t *pt_blob, uint8_t *ok, size_t n, int device);
int circl_hip_hpke_export(int kdf, int kem, int aead, CIRCL_HIP_HPKE_ROWS_, const uint8_t *exp_blob, const uint64_t *exp_off, size_t L, uint8_t *out, size_t n,
                          int device);
int circl_hip_hpke_seal_single(CIRCL_HIP_HPKE_SENDER_, CIRCL_HIP_HPKE_SEAL_, uint8_t *enc, uint8_t *ct_blob, uint8_t *ok, size_t n, int device);
int circl_hip_hpke_open_single(CIRCL_HIP_HPKE_RECEIVER_, CIRCL_HIP_HPKE_OPEN_, uint8_t *pt_blob, uint8_t *ok, size_t n, int device);
int circl_hip_hpke_export_single(CIRCL_HIP_HPKE_SENDER_, const uint8_t *exp_blob, const uint64_t *exp_off, size_t L, uint8_t *enc, uint8_t *out, uint8_t *ok,
                                 size_t n, int device);
int circl_hip_hpke_export_single_receiver(CIRCL_HIP_HPKE_RECEIVER_, const uint8_t *exp_blob, const uint64_t *exp_off, size_t L, uint8_t *out, uint8_t *ok,
                                          size_t n, int device);
/* the device-resident forms: the same arguments as device pointers, on the caller's stream */
int circl_hip_hpke_setup_sender_dev(CIRCL_HIP_HPKE_SENDER_, uint8_t *enc, uint8_t *ctx, uint8_t *ok, size_t n, void *stream);
int circl_hip_hpke_setup_receiver_dev(CIRCL_HIP_HPKE_RECEIVER_, uint8_t *ctx, uint8_t *ok, size_t n, void *stream);
int circl_hip_hpke_seal_dev(int aead, CIRCL_HIP_HPKE_ROWS_, const uint64_t *seq, CIRCL_HIP_HPKE_SEAL_, uint8_t *ct_blob, size_t n, void *stream);
int circl_hip_hpke_open_dev(int aead, CIRCL_HIP_HPKE_ROWS_, const uint64_t *seq, CIRCL_HIP_HPKE_OPEN_, uint8_t *pt_blob, uint8_t *ok, size_t n, void *stream);
int circl_hip_hpke_export_dev(int kdf, int kem, int aead, CIRCL_HIP_HPKE_ROWS_, const uint8_t *exp_blob, const uint64_t *exp_off, size_t L, uint8_t *out,
                              size_t n, void *stream);
int circl_hip_hpke_seal_single_dev(CIRCL_HIP_HPKE_SENDER_, CIRCL_HIP_HPKE_SEAL_, uint8_t *enc, uint8_t *ct_blob, uint8_t *ok, size_t n, void *stream);
int circl_hip_hpke_open_single_dev(CIRCL_HIP_HPKE_RECEIVER_, CIRCL_HIP_HPKE_OPEN_, uint8_t *pt_blob, uint8_t *ok, size_t n, void *stream);
int circl_hip_hpke_export_single_dev(CIRCL_HIP_HPKE_SENDER_, const uint8_t *exp_blob, const uint64_t *exp_off, size_t L, uint8_t *enc, uint8_t *out,
                                     uint8_t *ok, size_t n, void *stream);
int circl_hip_hpke_export_single_receiver_dev(CIRCL_HIP_HPKE_RECEIVER_, const uint8_t *exp_blob, const uint64_t *exp_off, size_t L, uint8_t *out, uint8_t *ok,
                                              size_t n, void *stream);
#undef CIRCL_HIP_HPKE_SENDER_
#undef CIRCL_HIP_HPKE_RECEIVER_
#undef CIRCL_HIP_HPKE_SEAL_
#undef CIRCL_HIP_HPKE_OPEN_
#undef CIRCL_HIP_HPKE_ROWS_

/* ---- ristretto255 (group/ristretto255.go; RFC 9496) and base-mode OPRF (oprf/keys.go, client.go, server.go; RFC 9497, suite
 * ristretto255-SHA512) --------------------------------------------------------------------------------------------------------
 * One item per lane, one launch per call, no workspace.  Elements and scalars are rows of 32 bytes (the canonical encodings),
 * OPRF outputs rows of 64.  Ragged arguments (messages, infos, inputs) are a blob and n + 1 uint64_t offsets; a NULL blob means that
 * every item's is empty (its offsets are then not read); a blob without offsets is CIRCL_HIP_EPARAM.
 * DECODING IS STRICT RFC 9496: an element encoding with s >= p, with bit 255 set, a negative s, a non-square, a negative t or
 * y = 0 is refused, and so is a scalar >= L.  The reference reduces s >= p and ignores bit 255 (its own test comments out the two
 * vectors); this is the one place where an item the reference accepts gets ok = 0.
 *   hash_to_group / hash_to_scalar:  Ristretto255.HashToElement / HashToScalar(msg_i, dst): expand_message_xmd (RFC 9380, SHA-512,
 *                    64 bytes), ONE dst for the batch, given as HOST bytes in both forms, 1 <= dst_len <= 255 (else
 *                    CIRCL_HIP_EPARAM; RFC 9380's rule for a longer tag is out of scope).
 *   scalar_mult:     out_i = scalar_i elem_i; scalar_stride = 32, or 0 for one scalar for the batch; elems == NULL: the generator
 *                    (fixed-base comb); flags & 1: by the scalar's inverse (other flag bits: CIRCL_HIP_EPARAM).  ok = 0 where the
 *                    element does not decode, the scalar is >= L or an inverse of zero is asked.  The identity is accepted here.
 *   derive_keypair:  DeriveKey(mode, seed_i, info_i), modes 0 (OPRF), 1 (VOPRF), 2 (POPRF); ok = 0 for an info over 65535 bytes or
 *                    where no counter gives a non-zero scalar.
 *   blind:           Client.DeterministicBlind, the same in modes 0, 1, 2 up to the tag: blinded_i = blind_i HashToGroup(input_i).
 *                    The library has no RNG: the caller draws the blinds.  ok = 0 for a blind that is zero or >= L, an input over
 *                    65535 bytes (RFC 9497 forbids it; the reference would truncate its length) or an identity element.
 *   evaluate:        base-mode Server.Evaluate: evaluated_i = sk blinded_i; sk_stride = 32, or 0 for the server's ONE key (staged
 *                    once per chunk, never copied n times).  ok = 0 where the blinded element does not decode or is the identity
 *                    (DeserializeElement), or the key is zero or >= L.
 *   finalize:        base-mode Client.Finalize: SHA-512(I2OSP(len, 2) || input_i || I2OSP(32, 2) || blind_i^-1 evaluated_i ||
 *                    "Finalize"); ok = 0 as for blind and evaluate.
 *   full_evaluate:   Server.FullEvaluate (mode 0) / VerifiableServer.FullEvaluate (mode 1) in ONE kernel: neither the hashed point nor
 *                    the evaluated element reaches memory.  Mode 2 needs the info tweak: CIRCL_HIP_EPARAM.
 * evaluate and finalize take no mode: they are base mode; the verifiable modes are served by the DLEQ block below.
 * ok[i] = 0 means every output row of item i is all zero.  ok may be NULL.  Any other mode, stride or flag is CIRCL_HIP_EPARAM,
 * reported before a device is looked for.  Keys, blinds, seeds, inputs and outputs are wiped from the host forms' staging; the _dev
 * forms want 4-byte aligned rows and 8-byte aligned offsets (CIRCL_HIP_EWORKSPACE otherwise).  n == 0 is CIRCL_HIP_OK. */
#define CIRCL_HIP_OPRF_MODE_OPRF 0
#define CIRCL_HIP_OPRF_MODE_VOPRF 1
#define CIRCL_HIP_OPRF_MODE_POPRF 2
#define CIRCL_HIP_R255_INVERT 1u /* scalar_mult flags */
int circl_hip_ristretto255_hash_to_group(const uint8_t *msg_blob, const uint64_t *msg_off, const uint8_t *dst, size_t dst_len, uint8_t *out, size_t n, int device);
int circl_hip_ristretto255_hash_to_scalar(const uint8_t *msg_blob, const uint64_t *msg_off, const uint8_t *dst, size_t dst_len, uint8_t *out, size_t n, int device);
int circl_hip_ristretto255_scalar_mult(const uint8_t *scalars, size_t scalar_stride, const uint8_t *elems, uint32_t flags, uint8_t *out, uint8_t *ok, size_t n,
                                       int device);
int circl_hip_oprf_derive_keypair(int mode, const uint8_t *seeds, const uint8_t *info_blob, const uint64_t *info_off, uint8_t *sk, uint8_t *pk, uint8_t *ok,
                                  size_t n, int device);
int circl_hip_oprf_blind(int mode, const uint8_t *input_blob, const uint64_t *input_off, const uint8_t *blinds, uint8_t *blinded, uint8_t *ok, size_t n, int device);
int circl_hip_oprf_evaluate(const uint8_t *sk, size_t sk_stride, const uint8_t *blinded, uint8_t *evaluated, uint8_t *ok, size_t n, int device);
int circl_hip_oprf_finalize(const uint8_t *input_blob, const uint64_t *input_off, const uint8_t *blinds, const uint8_t *evaluated, uint8_t *out, uint8_t *ok,
                            size_t n, int device);
int circl_hip_oprf_full_evaluate(int mode, const uint8_t *sk, size_t sk_stride, const uint8_t *input_blob, const uint64_t *input_off, uint8_t *out, uint8_t *ok,
                                 size_t n, int device);
/* the device-resident forms: the same arguments as device pointers (dst stays host bytes), on the caller's stream */
int circl_hip_ristretto255_hash_to_group_dev(const uint8_t *msg_blob, const uint64_t *msg_off, const uint8_t *dst, size_t dst_len, uint8_t *out, size_t n, void *stream);
int circl_hip_ristretto255_hash_to_scalar_dev(const uint8_t *msg_blob, const uint64_t *msg_off, const uint8_t *dst, size_t dst_len, uint8_t *out, size_t n, void *stream);
int circl_hip_ristretto255_scalar_mult_dev(const uint8_t *scalars, size_t scalar_stride, const uint8_t *elems, uint32_t flags, uint8_t *out, uint8_t *ok, size_t n,
                                       void *stream);
int circl_hip_oprf_derive_keypair_dev(int mode, const uint8_t *seeds, const uint8_t *info_blob, const uint64_t *info_off, uint8_t *sk, uint8_t *pk, uint8_t *ok,
                                  size_t n, void *stream);
int circl_hip_oprf_blind_dev(int mode, const uint8_t *input_blob, const uint64_t *input_off, const uint8_t *blinds, uint8_t *blinded, uint8_t *ok, size_t n, void *stream);
int circl_hip_oprf_evaluate_dev(const uint8_t *sk, size_t sk_stride, const uint8_t *blinded, uint8_t *evaluated, uint8_t *ok, size_t n, void *stream);
int circl_hip_oprf_finalize_dev(const uint8_t *input_blob, const uint64_t *input_off, const uint8_t *blinds, const uint8_t *evaluated, uint8_t *out, uint8_t *ok,
                            size_t n, void *stream);
int circl_hip_oprf_full_evaluate_dev(int mode, const uint8_t *sk, size_t sk_stride, const uint8_t *input_blob, const uint64_t *input_off, uint8_t *out, uint8_t *ok,
                                 size_t n, void *stream);

/* ---- NIST P-256 / P-384 (group/short.go; SEC 1, RFC 9380) and base-mode OPRF on them (RFC 9497, suites P256-SHA256 and
 * P384-SHA384) --------------------------------------------------------------------------------------------------------------------
 * The operations of the ristretto255 block above, on a curve chosen per call: curve = CIRCL_HIP_P256 or CIRCL_HIP_P384, anything else
 * is CIRCL_HIP_EPARAM.  One item per lane, one launch per call, no workspace.  Row shapes, for P-256 / P-384:
 *   scalars, keys, blinds   BIG-ENDIAN rows of Ns = 32 / 48 bytes; a stride is Ns, or 0 for one row for the batch
 *   elements                packed rows of Ne = 33 / 49 bytes, the SEC 1 COMPRESSED form 02|03 || x; no alignment is asked for
 *   seeds                   rows of 32
 *   OPRF outputs            rows of Nh = 32 / 48 (SHA-256 / SHA-384)
 * THE ONE DIFFERENCE FROM THE REFERENCE: only the compressed form is accepted (the reference also reads the uncompressed 04 || x || y),
 * and the identity, which SEC 1 writes as the single byte 00, is the all-zero row.  Decoding is strict: a prefix other than 02 / 03,
 * x >= p, or an x^3 - 3x + b that is not a square is refused, and so is a scalar >= n.
 * The rules of the ristretto255 block carry over: ragged blobs with n + 1 offsets, a NULL blob meaning every item's is empty, a blob
 * without offsets CIRCL_HIP_EPARAM; ONE host-side dst for the batch, 1..255 bytes; inputs and infos of at most 65535 bytes, else
 * ok = 0; ok[i] = 0 means every output row of item i is all zero; ok may be NULL; n == 0 is CIRCL_HIP_OK; secrets are wiped from the
 * host forms' staging; the contract is checked before a device is looked for.
 *   hash_to_group:   HashToElement(msg_i, dst) (two maps, added); flags & 1: HashToElementNonUniform (one map).  expand_message_xmd
 *                    over SHA-256 / SHA-384, L = 48 / 72, simplified SWU with Z = -10 / -12.
 *   hash_to_scalar:  HashToScalar(msg_i, dst): one L-byte value mod n.
 *   scalar_mult:     out_i = scalar_i elem_i; elems == NULL: the generator; flags & 1: by the scalar's inverse.  The identity is
 *                    accepted, in and out, with ok = 1.  ok = 0 where the element does not decode, the scalar is >= n or an inverse
 *                    of zero is asked.
 *   derive_keypair, blind, evaluate, finalize, full_evaluate: as in the ristretto255 block, with the context string
 *                    "OPRFV1-" || mode || "-P256-SHA256" / "-P384-SHA384", I2OSP(Ne, 2) in the Finalize hash, modes 0, 1, 2 (full_evaluate:
 *                    0, 1; 2 is CIRCL_HIP_EPARAM).  full_evaluate keeps the hashed point and the evaluated element out of memory.
 * The _dev forms want 4-byte aligned scalar, seed, sk and output rows and 8-byte aligned offsets (CIRCL_HIP_EWORKSPACE otherwise);
 * element rows may lie anywhere.  The DLEQ proofs and the mode-2 (POPRF) items on these curves are the circl_hip_nistp_dleq_* /
 * circl_hip_oprf_nistp_poprf_* block further down.  OUT OF SCOPE: P-521, the Go bridge. */
#define CIRCL_HIP_P256 256
#define CIRCL_HIP_P384 384
#define CIRCL_HIP_NISTP_NONUNIFORM 1u /* hash_to_group flags */
#define CIRCL_HIP_NISTP_INVERT 1u     /* scalar_mult flags */
int circl_hip_nistp_hash_to_group(int curve, const uint8_t *msg_blob, const uint64_t *msg_off, const uint8_t *dst, size_t dst_len, uint32_t flags, uint8_t *out,
                                  size_t n, int device);
int circl_hip_nistp_hash_to_scalar(int curve, const uint8_t *msg_blob, const uint64_t *msg_off, const uint8_t *dst, size_t dst_len, uint8_t *out, size_t n, int device);
int circl_hip_nistp_scalar_mult(int curve, const uint8_t *scalars, size_t scalar_stride, const uint8_t *elems, uint32_t flags, uint8_t *out, uint8_t *ok, size_t n,
                                int device);
int circl_hip_oprf_nistp_derive_keypair(int curve, int mode, const uint8_t *seeds, const uint8_t *info_blob, const uint64_t *info_off, uint8_t *sk, uint8_t *pk,
                                        uint8_t *ok, size_t n, int device);
int circl_hip_oprf_nistp_blind(int curve, int mode, const uint8_t *input_blob, const uint64_t *input_off, const uint8_t *blinds, uint8_t *blinded, uint8_t *ok,
                               size_t n, int device);
int circl_hip_oprf_nistp_evaluate(int curve, const uint8_t *sk, size_t sk_stride, const uint8_t *blinded, uint8_t *evaluated, uint8_t *ok, size_t n, int device);
int circl_hip_oprf_nistp_finalize(int curve, const uint8_t *input_blob, const uint64_t *input_off, const uint8_t *blinds, const uint8_t *evaluated, uint8_t *out,
                                  uint8_t *ok, size_t n, int device);
int circl_hip_oprf_nistp_full_evaluate(int curve, int mode, const uint8_t *sk, size_t sk_stride, const uint8_t *input_blob, const uint64_t *input_off, uint8_t *out,
                                       uint8_t *ok, size_t n, int device);
/* the device-resident forms: the same arguments as device pointers (dst stays host bytes), on the caller's stream */
int circl_hip_nistp_hash_to_group_dev(int curve, const uint8_t *msg_blob, const uint64_t *msg_off, const uint8_t *dst, size_t dst_len, uint32_t flags, uint8_t *out,
                                      size_t n, void *stream);
int circl_hip_nistp_hash_to_scalar_dev(int curve, const uint8_t *msg_blob, const uint64_t *msg_off, const uint8_t *dst, size_t dst_len, uint8_t *out, size_t n,
                                       void *stream);
int circl_hip_nistp_scalar_mult_dev(int curve, const uint8_t *scalars, size_t scalar_stride, const uint8_t *elems, uint32_t flags, uint8_t *out, uint8_t *ok, size_t n,
                                    void *stream);
int circl_hip_oprf_nistp_derive_keypair_dev(int curve, int mode, const uint8_t *seeds, const uint8_t *info_blob, const uint64_t *info_off, uint8_t *sk, uint8_t *pk,
                                            uint8_t *ok, size_t n, void *stream);
int circl_hip_oprf_nistp_blind_dev(int curve, int mode, const uint8_t *input_blob, const uint64_t *input_off, const uint8_t *blinds, uint8_t *blinded, uint8_t *ok,
                                   size_t n, void *stream);
int circl_hip_oprf_nistp_evaluate_dev(int curve, const uint8_t *sk, size_t sk_stride, const uint8_t *blinded, uint8_t *evaluated, uint8_t *ok, size_t n, void *stream);
int circl_hip_oprf_nistp_finalize_dev(int curve, const uint8_t *input_blob, const uint64_t *input_off, const uint8_t *blinds, const uint8_t *evaluated, uint8_t *out,
                                      uint8_t *ok, size_t n, void *stream);
int circl_hip_oprf_nistp_full_evaluate_dev(int curve, int mode, const uint8_t *sk, size_t sk_stride, const uint8_t *input_blob, const uint64_t *input_off,
                                           uint8_t *out, uint8_t *ok, size_t n, void *stream);

/* ---- batch DLEQ proofs (zk/dleq, the ...RFC9497 forms: fixed generator, the base not bound; RFC 9497 section 2.2) on ristretto255,
 * and the mode-2 (POPRF) items of oprf/client.go and oprf/server.go -------------------------------------------------------------
 * THE BATCH SHAPE.  A call carries n_req REQUESTS over flat arrays of elements (rows of 32 bytes) and req_off: n_req + 1 uint64_t
 * offsets counted in ELEMENTS; request g owns elements [req_off[g], req_off[g+1]).  Per-request arguments are rows indexed by g:
 * keys k, public keys kA, proof randomness r (32 bytes each), proofs (64 bytes: c || s) and ok.  k and kA may be shared by the call
 * (stride 0) or per request (stride 32); any other stride is CIRCL_HIP_EPARAM.  One proof per request:
 *   seed = SHA-512(I2(32) || kA || I2(len) || "Seed-" || dst),  d_j = HashToScalar(I2(64) || seed || I2(j) || I2(32) || B_j || I2(32) ||
 *   kB_j || "Composite"),  M = sum d_j B_j,  Z = k M (prover) or sum d_j kB_j (verifier),  c = HashToScalar(I2(32) || kA || .. M .. Z ..
 *   t2 .. t3 || "Challenge"),  both hashes under the tag "HashToScalar-" || dst;  prover: t2 = r G, t3 = r M, s = r - c k;  verifier:
 *   t2 = s G + c kA, t3 = s M + c Z, accept iff the recomputed c equals c.
 *   prove:   ProveBatchWithRandomnessRFC9497(k, kA, B, kB, r) per request.  kA is the caller's: a wrong kA yields a proof that does not
 *            verify, nothing worse.  The library has no RNG: the caller draws r, as it draws blinds.
 *   verify:  VerifyBatchRFC9497(kA, B, kB, proof) per request; ok[g] is the verdict (ok is required).
 * FAILURE IS A MASK: a failed request gets ok[g] = 0 and (prove) an all-zero proof row, and never disturbs another request.  A request
 * fails with 0 elements (ErrInvalidBatch) or more than 65535 (the index j travels as two bytes; the reference's uint16(j) would wrap
 * silently); with k or r zero or >= L (THE ONE DELIBERATE DIFFERENCE from the reference, which does not test r: r = 0 hands out
 * s = -c k); with kA or any element that does not decode (strict RFC 9496, as above); verification also with c or s >= L.
 * flags bit 0, CIRCL_HIP_DLEQ_NO_IDENTITY: an element that is the identity (32 zero bytes) fails the request (DeserializeElement; the
 * OPRF layer sets it); without it the identity is accepted, as zk/dleq accepts it.  Other flag bits are CIRCL_HIP_EPARAM.
 * dst is the caller's tag (the reference's Params.DST), HOST bytes in both forms, 0 <= dst_len <= 242 (so that the hash tag fits 255
 * bytes), else CIRCL_HIP_EPARAM.  The host forms check that req_off starts at 0 and never decreases (CIRCL_HIP_EPARAM).  The argument
 * contract is reported before a device is looked for.  n_req == 0 is CIRCL_HIP_OK.  The _dev forms take device pointers (4-byte aligned
 * rows, 8-byte aligned offsets and workspace), n_elems = req_off[n_req] - req_off[0] given explicitly, and a workspace of at least
 * dleq_workspace_size(n_req, n_elems) bytes (monotone in both; about 5 bytes per element plus 320 per request; nothing secret is
 * ever written to it), else CIRCL_HIP_EWORKSPACE.  k and r are wiped from the host forms' staging.
 * OUT OF SCOPE: the bound-base Prove / VerifyBatch forms with a caller's base A; P-521 (P-256 and P-384 are the block after this one);
 * the Go bridge.
 *   poprf_tweak:          secretFromInfo / pointFromInfo, m_i = HashToScalar("Info" || I2(len) || info_i).  With sk (pkS NULL), the
 *                         server's side: t = sk + m, t_inv = t^-1, tweaked = t G; ok = 0 for t = 0 (ErrInverseZero) or sk zero or >= L.
 *                         With pkS (sk NULL; t and t_inv not written), the client's: tweaked = m G + pkS; ok = 0 if that is the identity
 *                         or pkS does not decode.  Both or neither: CIRCL_HIP_EPARAM.  An info over 65535 bytes is ok = 0.  Strides: 0
 *                         (one key for the call) or 32.  t and t_inv are secret outputs.
 *   poprf_finalize:       PartialObliviousClient.Finalize without the proof: SHA-512(I2(len) || input_i || I2(len) || info_i || I2(32) ||
 *                         blind_i^-1 evaluated_i || "Finalize"); ok as for the base-mode finalize.
 *   poprf_full_evaluate:  PartialObliviousServer.FullEvaluate in one kernel: evaluates with (sk + m_i)^-1. */
#define CIRCL_HIP_DLEQ_NO_IDENTITY 1u
size_t circl_hip_dleq_workspace_size(size_t n_req, size_t n_elems);
int circl_hip_dleq_prove(const uint8_t *k, size_t k_stride, const uint8_t *kA, size_t kA_stride, const uint8_t *B, const uint8_t *kB, const uint64_t *req_off,
                         const uint8_t *r, const uint8_t *dst, size_t dst_len, uint32_t flags, uint8_t *proofs, uint8_t *ok, size_t n_req, int device);
int circl_hip_dleq_verify(const uint8_t *kA, size_t kA_stride, const uint8_t *B, const uint8_t *kB, const uint64_t *req_off, const uint8_t *proofs,
                          const uint8_t *dst, size_t dst_len, uint32_t flags, uint8_t *ok, size_t n_req, int device);
int circl_hip_dleq_prove_dev(const uint8_t *k, size_t k_stride, const uint8_t *kA, size_t kA_stride, const uint8_t *B, const uint8_t *kB, const uint64_t *req_off,
                             const uint8_t *r, const uint8_t *dst, size_t dst_len, uint32_t flags, uint8_t *proofs, uint8_t *ok, size_t n_req, size_t n_elems,
                             void *d_workspace, size_t workspace_bytes, void *stream);
int circl_hip_dleq_verify_dev(const uint8_t *kA, size_t kA_stride, const uint8_t *B, const uint8_t *kB, const uint64_t *req_off, const uint8_t *proofs,
                              const uint8_t *dst, size_t dst_len, uint32_t flags, uint8_t *ok, size_t n_req, size_t n_elems, void *d_workspace,
                              size_t workspace_bytes, void *stream);
int circl_hip_oprf_poprf_tweak(const uint8_t *sk, size_t sk_stride, const uint8_t *pkS, size_t pk_stride, const uint8_t *info_blob, const uint64_t *info_off,
                               uint8_t *t, uint8_t *t_inv, uint8_t *tweaked, uint8_t *ok, size_t n, int device);
int circl_hip_oprf_poprf_finalize(const uint8_t *input_blob, const uint64_t *input_off, const uint8_t *info_blob, const uint64_t *info_off, const uint8_t *blinds,
                                  const uint8_t *evaluated, uint8_t *out, uint8_t *ok, size_t n, int device);
int circl_hip_oprf_poprf_full_evaluate(const uint8_t *sk, size_t sk_stride, const uint8_t *input_blob, const uint64_t *input_off, const uint8_t *info_blob,
                                       const uint64_t *info_off, uint8_t *out, uint8_t *ok, size_t n, int device);
int circl_hip_oprf_poprf_tweak_dev(const uint8_t *sk, size_t sk_stride, const uint8_t *pkS, size_t pk_stride, const uint8_t *info_blob, const uint64_t *info_off,
                                   uint8_t *t, uint8_t *t_inv, uint8_t *tweaked, uint8_t *ok, size_t n, void *stream);
int circl_hip_oprf_poprf_finalize_dev(const uint8_t *input_blob, const uint64_t *input_off, const uint8_t *info_blob, const uint64_t *info_off,
                                      const uint8_t *blinds, const uint8_t *evaluated, uint8_t *out, uint8_t *ok, size_t n, void *stream);
int circl_hip_oprf_poprf_full_evaluate_dev(const uint8_t *sk, size_t sk_stride, const uint8_t *input_blob, const uint64_t *input_off, const uint8_t *info_blob,
                                           const uint64_t *info_off, uint8_t *out, uint8_t *ok, size_t n, void *stream);

/* ---- batch DLEQ proofs and the mode-2 (POPRF) items on NIST P-256 / P-384 (zk/dleq with Params{G, H: SHA-256 / SHA-384, DST}; RFC 9497
 * suites P256-SHA256 and P384-SHA384) ---------------------------------------------------------------------------------------------
 * The ristretto255 DLEQ block above, on a curve chosen per call: curve = CIRCL_HIP_P256 or CIRCL_HIP_P384 comes first, anything else is
 * CIRCL_HIP_EPARAM (nistp_dleq_workspace_size returns 0); the other arguments are those of the ristretto255 entry point of the same
 * name.  Row shapes follow the NIST block, for P-256 / P-384:
 *   k, r, t, t_inv, blinds   BIG-ENDIAN rows of Ns = 32 / 48 bytes; the k and sk strides are 0 (one key for the call) or Ns
 *   kA, B, kB, pkS, tweaked  packed SEC 1 COMPRESSED rows of Ne = 33 / 49 bytes; the kA and pkS strides are 0 or Ne
 *   proofs                   c || s, 2 Ns = 64 / 96 bytes, as Proof.MarshalBinary writes them
 *   OPRF outputs             Nh = 32 / 48 bytes
 * req_off counts ELEMENTS.  The transcript is the one above with the suite's hash, I2(Ne) in front of every element, I2(Nh) in front of
 * the seed, and HashToScalar = expand_message_xmd to L = 48 / 72 bytes reduced mod n.  The mode-2 context string is "OPRFV1-" || 2 ||
 * "-P256-SHA256" / "-P384-SHA384".
 * THE CONTRACT CARRIES OVER UNCHANGED: it is checked before a device is looked for; dst is host bytes in both forms, 0 <= dst_len <=
 * 242; the only flag bit is CIRCL_HIP_DLEQ_NO_IDENTITY; the host forms check that req_off starts at 0 and never decreases; the _dev
 * forms want 4-byte aligned scalar and proof rows and 8-byte aligned offsets and workspace (element rows may lie anywhere), n_elems
 * given explicitly and a workspace of nistp_dleq_workspace_size(curve, n_req, n_elems) bytes (CIRCL_HIP_EWORKSPACE otherwise; nothing
 * secret is written to it); n_req == 0 is CIRCL_HIP_OK; failure is a mask (ok = 0 and zero rows, neighbours untouched); k, r, t, t_inv
 * and the client's inputs are wiped from the host forms' staging.
 * THE DELIBERATE DIFFERENCES FROM THE REFERENCE, as above and in the NIST block: a request of 0 or of more than 65535 pairs fails; k or r
 * that is zero or >= n fails (the reference does not test r); verification fails with c or s >= n; only COMPRESSED encodings are accepted
 * (decoding is strict: prefix 02 / 03, x < p, on the curve); the identity is the all-zero row.
 * The launches are profiled under the ids of the ristretto255 launches of the same operation (37..41).
 * OUT OF SCOPE: P-521; the bound-base Prove / VerifyBatch forms; the Go bridge.  circl_hip_oprf_nistp_full_evaluate keeps refusing
 * mode 2: mode 2 is circl_hip_oprf_nistp_poprf_full_evaluate. */
size_t circl_hip_nistp_dleq_workspace_size(int curve, size_t n_req, size_t n_elems);
int circl_hip_nistp_dleq_prove(int curve, const uint8_t *k, size_t k_stride, const uint8_t *kA, size_t kA_stride, const uint8_t *B, const uint8_t *kB,
                               const uint64_t *req_off, const uint8_t *r, const uint8_t *dst, size_t dst_len, uint32_t flags, uint8_t *proofs, uint8_t *ok,
                               size_t n_req, int device);
int circl_hip_nistp_dleq_verify(int curve, const uint8_t *kA, size_t kA_stride, const uint8_t *B, const uint8_t *kB, const uint64_t *req_off, const uint8_t *proofs,
                                const uint8_t *dst, size_t dst_len, uint32_t flags, uint8_t *ok, size_t n_req, int device);
int circl_hip_nistp_dleq_prove_dev(int curve, const uint8_t *k, size_t k_stride, const uint8_t *kA, size_t kA_stride, const uint8_t *B, const uint8_t *kB,
                                   const uint64_t *req_off, const uint8_t *r, const uint8_t *dst, size_t dst_len, uint32_t flags, uint8_t *proofs, uint8_t *ok,
                                   size_t n_req, size_t n_elems, void *d_workspace, size_t workspace_bytes, void *stream);
int circl_hip_nistp_dleq_verify_dev(int curve, const uint8_t *kA, size_t kA_stride, const uint8_t *B, const uint8_t *kB, const uint64_t *req_off,
                                    const uint8_t *proofs, const uint8_t *dst, size_t dst_len, uint32_t flags, uint8_t *ok, size_t n_req, size_t n_elems,
                                    void *d_workspace, size_t workspace_bytes, void *stream);
int circl_hip_oprf_nistp_poprf_tweak(int curve, const uint8_t *sk, size_t sk_stride, const uint8_t *pkS, size_t pk_stride, const uint8_t *info_blob,
                                     const uint64_t *info_off, uint8_t *t, uint8_t *t_inv, uint8_t *tweaked, uint8_t *ok, size_t n, int device);
int circl_hip_oprf_nistp_poprf_finalize(int curve, const uint8_t *input_blob, const uint64_t *input_off, const uint8_t *info_blob, const uint64_t *info_off,
                                        const uint8_t *blinds, const uint8_t *evaluated, uint8_t *out, uint8_t *ok, size_t n, int device);
int circl_hip_oprf_nistp_poprf_full_evaluate(int curve, const uint8_t *sk, size_t sk_stride, const uint8_t *input_blob, const uint64_t *input_off,
                                             const uint8_t *info_blob, const uint64_t *info_off, uint8_t *out, uint8_t *ok, size_t n, int device);
int circl_hip_oprf_nistp_poprf_tweak_dev(int curve, const uint8_t *sk, size_t sk_stride, const uint8_t *pkS, size_t pk_stride, const uint8_t *info_blob,
                                         const uint64_t *info_off, uint8_t *t, uint8_t *t_inv, uint8_t *tweaked, uint8_t *ok, size_t n, void *stream);
int circl_hip_oprf_nistp_poprf_finalize_dev(int curve, const uint8_t *input_blob, const uint64_t *input_off, const uint8_t *info_blob, const uint64_t *info_off,
                                            const uint8_t *blinds, const uint8_t *evaluated, uint8_t *out, uint8_t *ok, size_t n, void *stream);
int circl_hip_oprf_nistp_poprf_full_evaluate_dev(int curve, const uint8_t *sk, size_t sk_stride, const uint8_t *input_blob, const uint64_t *input_off,
                                                 const uint8_t *info_blob, const uint64_t *info_off, uint8_t *out, uint8_t *ok, size_t n, void *stream);

/* ---- Ascon AEAD: Ascon128, Ascon128a, Ascon80pq (cipher/ascon/ascon.go; Ascon v1.2) ------------------------------------------
 * mode = the reference's Mode values.  One item per lane, one launch per call, no workspace.  Every other mode is
 * CIRCL_HIP_EPARAM, reported before a device is looked for, as is every breach of the rules below.
 * Keys are rows of circl_hip_ascon_key_size(mode) = 16 / 16 / 20 bytes (0 for an unknown mode), key_stride bytes apart (an array of
 * n key_stride bytes): key_stride == 0 means ONE key for the whole batch (the reference's New(key) and many Seal calls), otherwise
 * key_stride >= the key size and a multiple of 4.  Nonces are n rows of 16 bytes.  Keys are secret.
 * Ragged arguments (aad, plaintexts) are a blob and n + 1 uint64_t offsets; a NULL blob means that every item's input is empty
 * (its offsets are then not read).  Item i's plaintext is pt_off[i + 1] - pt_off[i] bytes at pt_blob[pt_off[i]]; its ciphertext
 * (ct || tag) is 16 bytes longer at ct_blob[pt_off[i] + 16 i]: the one offset array describes both sides.  The ciphertext blob of
 * Open is required (with pt_off == NULL it is n rows of 16: the tags of empty plaintexts).  Input and output blobs must not
 * overlap: the reference's in-place reuse of a buffer is not offered.
 *   seal: Cipher.Seal: initialize, assocData (an empty aad skips the absorb), procText, finalize -> ct || tag.
 *   open: Cipher.Open: decrypts and authenticates in one pass; the plaintext is written as it is computed and cleared when the tag
 *         does not verify.
 * ok[i] = 0 and the plaintext row of item i all zero where, for Open, the tag does not verify.  ok may be NULL.  The host forms zero
 * their staging; the _dev forms want 4-byte aligned key and nonce rows and 8-byte aligned offset arrays (CIRCL_HIP_EWORKSPACE
 * otherwise).  n == 0 is CIRCL_HIP_OK. */
#define CIRCL_HIP_ASCON128 1
#define CIRCL_HIP_ASCON128A 2
#define CIRCL_HIP_ASCON80PQ (-1)
size_t circl_hip_ascon_key_size(int mode);
int circl_hip_ascon_seal(int mode, const uint8_t *key, size_t key_stride, const uint8_t *nonce16, const uint8_t *pt_blob, const uint64_t *pt_off,
                         const uint8_t *aad_blob, const uint64_t *aad_off, uint8_t *ct_blob, size_t n, int device);
int circl_hip_ascon_open(int mode, const uint8_t *key, size_t key_stride, const uint8_t *nonce16, const uint8_t *ct_blob, const uint64_t *pt_off,
                         const uint8_t *aad_blob, const uint64_t *aad_off, uint8_t *pt_blob, uint8_t *ok, size_t n, int device);
/* the device-resident forms: the same arguments as device pointers, on the caller's stream */
int circl_hip_ascon_seal_dev(int mode, const uint8_t *key, size_t key_stride, const uint8_t *nonce16, const uint8_t *pt_blob, const uint64_t *pt_off,
                             const uint8_t *aad_blob, const uint64_t *aad_off, uint8_t *ct_blob, size_t n, void *stream);
int circl_hip_ascon_open_dev(int mode, const uint8_t *key, size_t key_stride, const uint8_t *nonce16, const uint8_t *ct_blob, const uint64_t *pt_off,
                             const uint8_t *aad_blob, const uint64_t *aad_off, uint8_t *pt_blob, uint8_t *ok, size_t n, void *stream);

/* ---- AES-GCM AEAD: AES-128-GCM, AES-256-GCM (hpke/aead.go's AEAD ids 1 and 2; NIST SP 800-38D over FIPS 197) -------------------
 * key_bytes = the key size, 16 or 32.  12-byte nonces, 16-byte tags.  One item per lane, one launch per call, no workspace.  Every
 * other key size (24 included: AES-192 is not served) is CIRCL_HIP_EPARAM, reported before a device is looked for, as is every
 * breach of the rules below.  AES and GHASH are constant-time software (the chip has neither an AES round nor a carry-less
 * multiply): no table is indexed by, and no branch depends on, a key, a plaintext, the hash key or a tag.
 * Keys are rows of key_bytes, key_stride bytes apart (an array of n key_stride bytes): key_stride == 0 means ONE key for the whole
 * batch, otherwise key_stride >= key_bytes and a multiple of 4.  Keys are secret.
 * Nonces are rows of 12 bytes, nonce_stride bytes apart (only the 12 bytes of a row are read): nonce_stride >= 12 and a multiple of
 * 4, or nonce_stride == 0 -- ONE base nonce for the whole batch -- which needs seq.  seq == NULL: the row is the nonce.  seq != NULL
 * (n sequence numbers): the nonce is the row XOR BE96(seq[i]), as hpke/aead.go computes it; one HPKE context sealing a run of
 * records is key_stride = nonce_stride = 0 and seq = first, first + 1, ...  With both strides free an array of HPKE-style context
 * rows (key || base_nonce || ...) is passed as it stands: key at +0, nonce12 at +32, both strides the row size (80 or 112).
 * Distinct (key, nonce) pairs are the CALLER's duty, as with Go's cipher.AEAD: nothing here detects a pair used twice, in a batch
 * or across calls, and a repeated pair gives away the xor of the plaintexts and the hash key.
 * Ragged arguments (aad, plaintexts) are a blob and n + 1 uint64_t offsets; a NULL blob means that every item's input is empty
 * (its offsets are then not read).  Item i's plaintext is pt_off[i + 1] - pt_off[i] bytes at pt_blob[pt_off[i]]; its ciphertext
 * (ct || tag) is 16 bytes longer at ct_blob[pt_off[i] + 16 i]: the one offset array describes both sides.  The ciphertext blob of
 * Open is required (with pt_off == NULL it is n rows of 16: the tags of empty plaintexts).  Input and output blobs must not
 * overlap: in-place operation is not offered.  A plaintext is at most 2^36 - 32 bytes (SP 800-38D 5.2.1.1): the host forms, which
 * read the offsets, refuse a longer one (and decreasing offsets); for the _dev forms that limit is the caller's to keep.
 *   seal: ct = pt XOR the keystream E_K(nonce || 2), E_K(nonce || 3), ... (inc32); tag = GHASH_H(aad, ct, lengths) XOR E_K(nonce || 1).
 *   open: authenticates the whole ciphertext first and decrypts under the verdict: no unauthenticated plaintext byte is written.
 * ok[i] = 0 and the plaintext row of item i all zero where, for Open, the tag does not verify.  ok may be NULL.  The host forms zero
 * their staging; the _dev forms want 4-byte aligned key and nonce rows and 8-byte aligned seq and offset arrays
 * (CIRCL_HIP_EWORKSPACE otherwise).  n == 0 is CIRCL_HIP_OK. */
#define CIRCL_HIP_AES128GCM 16 /* = the key size in bytes */
#define CIRCL_HIP_AES256GCM 32
int circl_hip_aesgcm_seal(int key_bytes, const uint8_t *key, size_t key_stride, const uint8_t *nonce12, size_t nonce_stride, const uint64_t *seq,
                          const uint8_t *pt_blob, const uint64_t *pt_off, const uint8_t *aad_blob, const uint64_t *aad_off, uint8_t *ct_blob, size_t n,
                          int device);
int circl_hip_aesgcm_open(int key_bytes, const uint8_t *key, size_t key_stride, const uint8_t *nonce12, size_t nonce_stride, const uint64_t *seq,
                          const uint8_t *ct_blob, const uint64_t *pt_off, const uint8_t *aad_blob, const uint64_t *aad_off, uint8_t *pt_blob, uint8_t *ok,
                          size_t n, int device);
/* the device-resident forms: the same arguments as device pointers, on the caller's stream */
int circl_hip_aesgcm_seal_dev(int key_bytes, const uint8_t *key, size_t key_stride, const uint8_t *nonce12, size_t nonce_stride, const uint64_t *seq,
                              const uint8_t *pt_blob, const uint64_t *pt_off, const uint8_t *aad_blob, const uint64_t *aad_off, uint8_t *ct_blob, size_t n,
                              void *stream);
int circl_hip_aesgcm_open_dev(int key_bytes, const uint8_t *key, size_t key_stride, const uint8_t *nonce12, size_t nonce_stride, const uint64_t *seq,
                              const uint8_t *ct_blob, const uint64_t *pt_off, const uint8_t *aad_blob, const uint64_t *aad_off, uint8_t *pt_blob, uint8_t *ok,
                              size_t n, void *stream);

/* ---- Prio3Count and Prio3Sum: batch VDAF preparation (the reference's vdaf/prio3/count and vdaf/prio3/sum) -------------------------
 * draft-irtf-cfrg-vdaf-13 section 7 over Field64 (p = 2^64 - 2^32 + 1) and XofTurboShake128, one report per lane.  A batch is n reports
 * under ONE task, spelled the same way in every call:
 *   kind             CIRCL_HIP_PRIO3_COUNT or CIRCL_HIP_PRIO3_SUM (the algorithm ids 1 and 2);
 *   max_measurement  0 for Count; 1 .. 2^63 - 1 for Sum (0 is refused: the reference accepts that degenerate type, this library does not);
 *   shares           2 .. 255 aggregators;
 *   ctx, ctx_len     the application context string, a HOST pointer in both forms (a task parameter like the scalars: it travels to the
 *                    kernels by value); ctx_len <= 255, a longer one is CIRCL_HIP_EPARAM (the reference allows 65527; DAP uses about 40).
 * Anything else is CIRCL_HIP_EPARAM, decided before a device is looked for; so are NULL pointers (ok may be NULL in shard and prep_init,
 * mask in aggregate).  n == 0 is CIRCL_HIP_OK.  All encodings are the reference's MarshalBinary: an element is 8 little-endian
 * bytes, canonical (< p).  Sizes, b = the bit length of max_measurement, P = the next power of two >= 1 + gadget calls:
 *   Count: leader share 8 (1 + 5) = 48 bytes, prep share 32;   Sum: leader share 8 (2b + 2P), prep share 24;   rand 32 shares;
 *   nonce 16, verify key 32, out share 8, aggregate share 8.  The size queries return 0 for a type that is not served.
 *
 *   shard        measurement[n] (uint64), rand[n][32 shares] (the seeds of helpers 1 .. shares - 1, then the prove seed, as the reference
 *                reads them) -> leader_share[n][..], ok[n].  Helper j's input share is bytes 32 (j - 1) .. 32 j of the caller's own rand
 *                row and is written nowhere.  ok = 0 and a zero row: a measurement out of range (Count > 1, Sum > max_measurement), or a
 *                sampler that was refused 10 words in a row.
 *   prep_init    agg_id (one per call, < shares), verify_key[32] (one per call), nonce[n][16], input_share[n][..] (the leader share for
 *                agg_id 0, otherwise the 32-byte seed) -> prep_share[n][..], out_share[n][8], ok[n].  The out share is the prepare
 *                state: without joint randomness PrepNext is the identity and the prep message is empty, so neither has a call.  ok = 0
 *                and zero rows: a leader share with an element that is not canonical, an evaluation point t with t^P = 1, an exhausted
 *                sampler.
 *   prep_finish  PrepSharesToPrep: prep_shares[n][shares x prep share], item-major, an item's shares in aggregator order -> ok[n], Decide
 *                on the summed verifier; an element that is not canonical is ok = 0.
 *   aggregate    AggregateUpdate over the batch: agg_share[8] (read and updated) += the out_share[n][8] with mask[i] != 0 (mask == NULL:
 *                all of them).  Exact modular sums: the result does not depend on the order.  Elements are reduced mod p as read.
 *   unshard      host only, looks for no device: agg_shares[shares][8], num_measurements -> *result, the reference's Decode.  For Sum,
 *                num_measurements x max_measurement that is not an element (ErrAggregateBound) is CIRCL_HIP_EPARAM, as is an aggregate share
 *                that is not canonical.
 * The _dev forms of shard, prep_init and aggregate take a workspace of circl_hip_prio3_workspace_size(kind, max_measurement, n) bytes
 * (monotone in n; 8 (2 arity P + 2b + 1) bytes per report rounded up to 64 reports, at least 8 KB; aggregate alone needs the 8 KB): the
 * reports' wires and folded polynomials, as secret afterwards as the call's inputs.  A workspace that is too small, or a pointer that is
 * not 8-byte aligned (ok and mask excepted), is CIRCL_HIP_EWORKSPACE.  The host forms allocate the workspace in the pipeline.
 * Measurements, rand, input shares, the verify key, out shares and the aggregate share are secret: the host forms wipe their staging
 * and zero the device staging of every chunk.  Nonces, prep shares and verdicts are not.
 * The launches run without a profiling scope: there is no CIRCL_HIP_KERNEL_* id for them.
 * Not served: Prio3SumVec, Prio3Histogram and Prio3MultihotCountVec (Field128, joint randomness, a workgroup per report); more than one
 * proof (the reference fixes it at 1 as well); key tables, the coalescer and the asynchronous queue; the Go bridge. */
#define CIRCL_HIP_PRIO3_COUNT 1
#define CIRCL_HIP_PRIO3_SUM 2
size_t circl_hip_prio3_leader_share_size(int kind, uint64_t max_measurement);
size_t circl_hip_prio3_prep_share_size(int kind);
size_t circl_hip_prio3_rand_size(int shares);
size_t circl_hip_prio3_workspace_size(int kind, uint64_t max_measurement, size_t n);
int circl_hip_prio3_shard(int kind, uint64_t max_measurement, int shares, const uint8_t *ctx, size_t ctx_len, const uint64_t *measurement, const uint8_t *rand,
                          uint8_t *leader_share, uint8_t *ok, size_t n, int device);
int circl_hip_prio3_prep_init(int kind, uint64_t max_measurement, int shares, const uint8_t *ctx, size_t ctx_len, int agg_id, const uint8_t *verify_key,
                              const uint8_t *nonce, const uint8_t *input_share, uint8_t *prep_share, uint8_t *out_share, uint8_t *ok, size_t n, int device);
int circl_hip_prio3_prep_finish(int kind, uint64_t max_measurement, int shares, const uint8_t *ctx, size_t ctx_len, const uint8_t *prep_shares, uint8_t *ok,
                                size_t n, int device);
int circl_hip_prio3_aggregate(int kind, uint64_t max_measurement, int shares, const uint8_t *ctx, size_t ctx_len, const uint8_t *out_share, const uint8_t *mask,
                              uint8_t *agg_share, size_t n, int device);
int circl_hip_prio3_unshard(int kind, uint64_t max_measurement, int shares, const uint8_t *ctx, size_t ctx_len, const uint8_t *agg_shares,
                            uint64_t num_measurements, uint64_t *result);
/* the device-resident forms: the same arguments as device pointers (ctx stays a host pointer), on the caller's stream */
int circl_hip_prio3_shard_dev(int kind, uint64_t max_measurement, int shares, const uint8_t *ctx, size_t ctx_len, const uint64_t *measurement,
                              const uint8_t *rand, uint8_t *leader_share, uint8_t *ok, size_t n, void *d_workspace, size_t workspace_bytes, void *stream);
int circl_hip_prio3_prep_init_dev(int kind, uint64_t max_measurement, int shares, const uint8_t *ctx, size_t ctx_len, int agg_id, const uint8_t *verify_key,
                                  const uint8_t *nonce, const uint8_t *input_share, uint8_t *prep_share, uint8_t *out_share, uint8_t *ok, size_t n,
                                  void *d_workspace, size_t workspace_bytes, void *stream);
int circl_hip_prio3_prep_finish_dev(int kind, uint64_t max_measurement, int shares, const uint8_t *ctx, size_t ctx_len, const uint8_t *prep_shares, uint8_t *ok,
                                    size_t n, void *stream);
int circl_hip_prio3_aggregate_dev(int kind, uint64_t max_measurement, int shares, const uint8_t *ctx, size_t ctx_len, const uint8_t *out_share,
                                  const uint8_t *mask, uint8_t *agg_share, size_t n, void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- kernel-level profiling (used by bench.py for the roofline figures) --------------------
 * While enabled, every *_dev call brackets each kernel it enqueues with HIP events recorded on
 * the caller's stream.  circl_hip_profile_read synchronises the pending events, returns the
 * accumulated device time and launch count of one kernel and resets that kernel's counters. */
#define CIRCL_HIP_KERNEL_MLKEM_HASH 0     /* H(ek), G(m||H(ek))                      */
#define CIRCL_HIP_KERNEL_MLKEM_ENCRYPT 1  /* matrix expansion + PRF + K-PKE.Encrypt  */
#define CIRCL_HIP_KERNEL_MLKEM_DECRYPT 2  /* K-PKE.Decrypt + G + J                   */
#define CIRCL_HIP_KERNEL_MLKEM_KEYGEN 3
#define CIRCL_HIP_KERNEL_MLKEM_FINISH 4   /* decapsulation compare / select          */
#define CIRCL_HIP_KERNEL_MLDSA_HASH 5
#define CIRCL_HIP_KERNEL_MLDSA_VERIFY 6
#define CIRCL_HIP_KERNEL_MLDSA_KEYGEN 7
#define CIRCL_HIP_KERNEL_MLDSA_SIGN 8
#define CIRCL_HIP_KERNEL_MLKEM_KEYTABLE 9  /* key tables: H(ek) + A^T per table entry */
#define CIRCL_HIP_KERNEL_MLDSA_KEYTABLE 10 /* key tables: tr + ExpandA per table entry */
#define CIRCL_HIP_KERNEL_X25519 11         /* X25519 ladder                            */
#define CIRCL_HIP_KERNEL_ED25519_KEYGEN 12 /* Ed25519 NewKeyFromSeed                   */
#define CIRCL_HIP_KERNEL_ED25519_SIGN 13   /* Ed25519 Sign                             */
#define CIRCL_HIP_KERNEL_ED25519_VERIFY 14 /* Ed25519 Verify                           */
#define CIRCL_HIP_KERNEL_SHA512 15         /* batch SHA-512                            */
#define CIRCL_HIP_KERNEL_X448 16           /* X448 ladder                              */
#define CIRCL_HIP_KERNEL_ED448_KEYGEN 17   /* Ed448 NewKeyFromSeed                     */
#define CIRCL_HIP_KERNEL_ED448_SIGN 18     /* Ed448 Sign                               */
#define CIRCL_HIP_KERNEL_ED448_VERIFY 19   /* Ed448 Verify                             */
#define CIRCL_HIP_KERNEL_FRODO_KEYGEN 20   /* FrodoKEM-640-SHAKE KeyGen (three launches) */
#define CIRCL_HIP_KERNEL_FRODO_ENCAPS 21   /* FrodoKEM-640-SHAKE Encaps                */
#define CIRCL_HIP_KERNEL_FRODO_DECAPS 22   /* FrodoKEM-640-SHAKE Decaps                */
#define CIRCL_HIP_KERNEL_HPKE_X25519 23    /* HPKE DHKEM(X25519, HKDF-SHA256), every operation */
#define CIRCL_HIP_KERNEL_HPKE_X448 24      /* HPKE DHKEM(X448, HKDF-SHA512), every operation   */
#define CIRCL_HIP_KERNEL_SHA256 25         /* batch SHA-256                            */
#define CIRCL_HIP_KERNEL_HPKE_SETUP 26     /* HPKE setup (DHKEM + key schedule) and the single-shot forms */
#define CIRCL_HIP_KERNEL_HPKE_AEAD 27      /* HPKE Seal / Open on context rows (ChaCha20-Poly1305) */
#define CIRCL_HIP_KERNEL_HPKE_EXPORT 28    /* HPKE Export on context rows              */
/* ids 29..36: the ristretto255 launches, and the circl_hip_nistp_* / circl_hip_oprf_nistp_* launches of the same operation */
#define CIRCL_HIP_KERNEL_OPRF_HASH_TO_GROUP 29   /* ristretto255 HashToElement      */
#define CIRCL_HIP_KERNEL_OPRF_HASH_TO_SCALAR 30  /* ristretto255 HashToScalar       */
#define CIRCL_HIP_KERNEL_OPRF_SCALAR_MULT 31     /* ristretto255 scalar multiplication */
#define CIRCL_HIP_KERNEL_OPRF_DERIVE_KEYPAIR 32  /* OPRF DeriveKey                  */
#define CIRCL_HIP_KERNEL_OPRF_BLIND 33           /* OPRF DeterministicBlind         */
#define CIRCL_HIP_KERNEL_OPRF_EVALUATE 34        /* OPRF Evaluate (base mode)       */
#define CIRCL_HIP_KERNEL_OPRF_FINALIZE 35        /* OPRF Finalize (base mode)       */
#define CIRCL_HIP_KERNEL_OPRF_FULL_EVALUATE 36   /* OPRF FullEvaluate               */
/* ids 37..41: the ristretto255 launches, and the circl_hip_nistp_dleq_* / circl_hip_oprf_nistp_poprf_* launches of the same operation */
#define CIRCL_HIP_KERNEL_DLEQ_COMPOSITE 37        /* DLEQ: d_j B_j per element, segmented sums */
#define CIRCL_HIP_KERNEL_DLEQ_FINISH 38           /* DLEQ: the prover's / verifier's tail per request */
#define CIRCL_HIP_KERNEL_OPRF_POPRF_TWEAK 39      /* POPRF secretFromInfo / pointFromInfo */
#define CIRCL_HIP_KERNEL_OPRF_POPRF_FINALIZE 40   /* POPRF Finalize                  */
#define CIRCL_HIP_KERNEL_OPRF_POPRF_FULL_EVALUATE 41 /* POPRF FullEvaluate           */
#define CIRCL_HIP_KERNEL_ASCON_SEAL 42             /* Ascon Seal                      */
#define CIRCL_HIP_KERNEL_ASCON_OPEN 43             /* Ascon Open                      */
#define CIRCL_HIP_KERNEL_AESGCM_SEAL 44            /* AES-GCM Seal                    */
#define CIRCL_HIP_KERNEL_AESGCM_OPEN 45            /* AES-GCM Open                    */
#define CIRCL_HIP_KERNEL_COUNT 46
int circl_hip_profile_enable(int on);
int circl_hip_profile_read(int kernel, double *total_ms, uint64_t *launches);
/* The VALU issue rates this chip sustains, measured live (bench.py prices the kernels' VALU time against them instead of against
 * figures of an earlier round): wave-instructions per second per SIMD of (a) the library's own Keccak-f[1600] round running on
 * register-resident states (keccak_dev.h: V_BITOP3 / V_ALIGNBIT, no memory traffic) and (b) two-operand integer VALU instructions
 * (the cheapest class), with `waves_per_simd` (1..8; the Keccak probe needs ~110 VGPRs, so at most 4 are resident) wavefronts
 * on every SIMD of `device`.  About 10 ms of GPU time.  Either output may be NULL. */
int circl_hip_profile_valu_probe(int device, int waves_per_simd, double *keccak_insts_per_s_per_simd, double *simple_insts_per_s_per_simd);
/* Where the microseconds of ONE blocking coalesced call go (profiles/r06_one_call.txt): enable != 0 switches the time stamps on, 0 off,
 * < 0 leaves the switch alone; out8 (may be NULL) receives the CLOCK_MONOTONIC nanoseconds of the calling thread's LAST blocking
 * coalesced call: [0] entered, [1] rows reserved, [2] own inputs copied in, and -- for the call that led its batch, else 0 -- [3] batch
 * closed (its turn, room on the device), [4] every caller's inputs in, [5] copies + kernels enqueued, [6] batch finished; [7] own results
 * copied out. */
int circl_hip_profile_call_stamps(int enable, uint64_t *out8);

/* What the host-buffer pipeline's staging pools hold right now, over all (logical) devices: slots created, page-locked host bytes,
 * device bytes.  The pools grow on demand (up to CIRCL_HIP_HOST_SLOTS slots per device) and are never shrunk: after a process's largest
 * calls this is the high-water mark a node has to budget for (profiles/r05_logical8.txt).  Any pointer may be NULL. */
int circl_hip_host_pool_stats(int *slots, uint64_t *pinned_bytes, uint64_t *device_bytes);

/* pinned host memory helpers for callers that want zero-copy-speed transfers */
void *circl_hip_alloc_host(size_t bytes);
void circl_hip_free_host(void *p);

#ifdef __cplusplus
}
#endif
#endif
