/*
 * kwgpu.h — C ABI of the MI355X batched admission-evaluation engine (libkwgpu.so).
 *
 * This is the drop-in boundary for the Kubewarden policy-server hot path
 *   POST /validate|/audit|/validate_raw/{policy_id}
 *     -> service::evaluate                      (src/api/service.rs:30-152)
 *     -> EvaluationEnvironment::validate        (src/evaluation/evaluation_environment.rs:546-556)
 * for the declarative policy class (namespace allow-list, trusted-repos, psp-capabilities,
 * psp-apparmor, safe-labels, pod-privileged, and policy groups over them).
 *
 * Every entry point names the reference interface it replaces. Plain pointers and sizes only:
 * no torch / HIP types appear in a signature ("stream" is an opaque hipStream_t or NULL).
 * All functions are thread-safe on a built (immutable) kw_env, like the reference's
 * Arc<EvaluationEnvironment> (src/lib.rs:194-197).
 */
#ifndef KWGPU_H
#define KWGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * Status codes. The first six mirror EvaluationError (src/evaluation/errors.rs:5-24) one to one;
 * the HTTP mapping of handle_evaluation_error (src/api/handlers.rs:321-342) is:
 * KW_E_NOT_FOUND -> 404 {"message":"unknown policy: <id>"}, every other error -> 500
 * {"message":"Something went wrong"}. KW_E_PAYLOAD is the 422 of JsonExtractor (handlers.rs:29-39).
 * ------------------------------------------------------------------------------------------- */
enum {
  KW_OK = 0,
  KW_E_INVALID_ID = 1,      /* EvaluationError::InvalidPolicyId        "Not a valid Policy ID: {0}" */
  KW_E_INIT = 2,            /* EvaluationError::PolicyInitialization   "{0}"                        */
  KW_E_NOT_FOUND = 3,       /* EvaluationError::PolicyNotFound         "unknown policy: {0}"        */
  KW_E_BOOTSTRAP = 4,       /* EvaluationError::BootstrapFailure       "bootstrap failure: {0}"     */
  KW_E_ENGINE = 5,          /* EvaluationError::WebAssemblyError slot: device/engine failure     */
  KW_E_GROUP_REHYDRATE = 6, /* EvaluationError::CannotRehydratePolicyGroup                        */
  KW_E_ARG = 16,            /* bad argument to this ABI                                           */
  KW_E_PAYLOAD = 17,        /* request JSON does not deserialize (HTTP 422)                       */
  KW_E_DEVICE = 18,         /* HIP runtime error                                                  */
  KW_E_NOSPACE = 19         /* caller buffer too small; *need holds the size                     */
};

/* PolicyMode (src/config.rs:287-294) */
enum { KW_MODE_PROTECT = 0, KW_MODE_MONITOR = 1 };
/* RequestOrigin (src/api/service.rs:16-19) */
enum { KW_ORIGIN_VALIDATE = 0, KW_ORIGIN_AUDIT = 1 };
/* ValidateRequest kind: AdmissionRequest vs Raw (service.rs:40, :134) */
enum { KW_DOC_ADMISSION_REVIEW = 0, KW_DOC_RAW_REVIEW = 1 };

/* ---------------------------------------------------------------------------------------------
 * Columnar (SoA) request batch. One row per ValidateRequest. Every string column is an offset
 * array (n+1 entries, u32) plus a byte pool; string i of a column belongs to entity i of that
 * column's table. Byte pools are padded to 16 B so device loads may over-read within the pad.
 * ------------------------------------------------------------------------------------------- */
typedef struct kw_strcol {
  const uint32_t *off;  /* n+1 offsets into bytes */
  const uint8_t *bytes; /* pool */
  uint64_t n;           /* number of strings */
} kw_strcol;

/* request flags */
enum {
  KW_REQ_RAW = 1u << 0,           /* ValidateRequest::Raw: namespace bypass is skipped (service.rs:40) */
  KW_REQ_HAS_NAMESPACE = 1u << 1, /* AdmissionRequest.namespace is Some */
  KW_REQ_HAS_PODSPEC = 1u << 2,   /* object carries a PodSpec (Pod or a workload template) */
  KW_REQ_HAS_OBJECT = 1u << 3     /* object is present and non-null */
};
/* container flags (containers, initContainers, ephemeralContainers, in that order) */
enum {
  KW_CTR_PRIVILEGED = 1u << 0,  /* securityContext.privileged == true */
  KW_CTR_INIT = 1u << 1,
  KW_CTR_EPHEMERAL = 1u << 2,
  KW_CTR_HAS_IMAGE = 1u << 3,
  KW_CTR_HAS_APPARMOR = 1u << 4 /* container.apparmor.security.beta.kubernetes.io/<name> annotation */
};

typedef struct kw_soa {
  uint64_t n_requests;
  /* per request */
  const uint8_t *req_flags; /* KW_REQ_* */
  const uint32_t *ctr_off;  /* n_requests+1: container range of each request */
  const uint32_t *lbl_off;  /* n_requests+1: metadata.labels range of each request */
  kw_strcol uid;            /* request.uid (host only, echoed in the response: service.rs:61,87) */
  kw_strcol ns;             /* request.namespace ("" when absent) */
  kw_strcol op;             /* request.operation */
  kw_strcol kind;           /* request.kind.kind */
  /* per container */
  const uint8_t *ctr_flags;   /* KW_CTR_* */
  const uint32_t *capadd_off; /* n_containers+1: securityContext.capabilities.add range */
  const uint32_t *capdrop_off;/* n_containers+1: securityContext.capabilities.drop range */
  kw_strcol ctr_name;
  kw_strcol ctr_image;
  kw_strcol ctr_apparmor; /* AppArmor profile from the pod annotation ("" when absent) */
  /* per capability entry */
  kw_strcol cap_add;
  kw_strcol cap_drop;
  /* per label */
  kw_strcol lbl_key;
  kw_strcol lbl_val;
} kw_soa;

/* ---------------------------------------------------------------------------------------------
 * Verdict word: one u32 per (row, policy) pair, written by the device.
 *   bit 0      V_ALLOWED   vanilla AdmissionResponse.allowed (the policy's own answer)
 *   bit 1      V_MUTATED   vanilla response carries a patch
 *   bit 2      F_ALLOWED   allowed after service::evaluate (bypass, init error, constraints)
 *   bits 3-4   F_STATUS    0: status None, 1: vanilla status, 2: mutation refused
 *                          (service.rs:168-180), 3: PolicyInitialization reject 500 (service.rs:78-91)
 *   bit 5      BYPASS      always-accept namespace (service.rs:40-71)
 *   bit 6      F_PATCH     the final response carries the vanilla patch (Audit, or Protect with
 *                          allowedToMutate)
 *   bits 8-15  REASON      kw_reason (0 = no violation)
 *   bits 16-31 ARG         reason argument: an entity index within the request, a settings index,
 *                          or a group's cause mask; KW_ARG_WIDE (0xffff) when the full value does
 *                          not fit (an index >= 65535, the causes of a group with more than 15
 *                          members): kw_batch_wide_arg returns it after kw_batch_verdicts
 * ------------------------------------------------------------------------------------------- */
#define KW_V_ALLOWED 0x1u
#define KW_V_MUTATED 0x2u
#define KW_F_ALLOWED 0x4u
#define KW_F_STATUS_SHIFT 3
#define KW_F_STATUS_MASK 0x18u
#define KW_BYPASS 0x20u
#define KW_F_PATCH 0x40u
#define KW_REASON(v) (((v) >> 8) & 0xffu)
#define KW_ARG(v) ((v) >> 16)
#define KW_ARG_WIDE 0xffffu
enum { KW_FST_NONE = 0, KW_FST_VANILLA = 1, KW_FST_MUTATION_REFUSED = 2, KW_FST_INIT_ERROR = 3 };

/* reason codes (message templates: DESIGN.md §Policy families) */
enum {
  KW_R_NONE = 0,
  KW_R_PRIVILEGED = 1,        /* arg: container index within the request */
  KW_R_NAMESPACE = 2,         /* namespace not the valid one */
  KW_R_REG_NOT_ALLOWED = 3,   /* arg: container index */
  KW_R_REG_REJECTED = 4,
  KW_R_TAG_REJECTED = 5,
  KW_R_IMG_NOT_ALLOWED = 6,
  KW_R_IMG_REJECTED = 7,
  KW_R_CAP_NOT_ALLOWED = 8,   /* arg: index in the request's capabilities.add lists, flattened in
                                 container order (the container is the one whose list holds it) */
  KW_R_APPARMOR = 9,          /* arg: container index */
  KW_R_LABEL_DENIED = 10,     /* arg: label index */
  KW_R_LABEL_CONSTRAINT = 11, /* arg: label index (the constraint is the policy's on that key) */
  KW_R_LABEL_MANDATORY = 12,  /* arg: index of the missing key in settings order */
  KW_R_GROUP = 13,            /* arg: cause mask over group members (settings order) */
  KW_R_GROUP_EXPR = 14,       /* group expression does not evaluate to a bool: reject 500 */
  KW_R_INIT_ERROR = 15
};

/* ---------------------------------------------------------------------------------------------
 * EvaluationEnvironment (src/evaluation/evaluation_environment.rs:86-127)
 * ------------------------------------------------------------------------------------------- */
typedef struct kw_env kw_env;

typedef struct kw_env_options {
  int continue_on_errors;              /* EvaluationEnvironmentBuilder::with_continue_on_errors :166 */
  const char *always_accept_namespace; /* ::with_always_accept_admission_reviews_on_namespace :172; NULL = None */
  int device;                          /* HIP device ordinal for the compiled tables; -1 = host only */
} kw_env_options;

/* EvaluationEnvironmentBuilder::build (evaluation_environment.rs:189-194, 198-332) plus the
 * policies.yml schema checks (src/config.rs:237-258, 287-453). `policies_json` is the policies file
 * as JSON (the reference converts YAML settings to JSON itself: config.rs:419-443). Compiles every
 * policy's settings into DFA/bitmask tables. On error returns the EvaluationError code and writes
 * its Display string into err. */
int kw_env_build(const char *policies_json, size_t len, const kw_env_options *opts, kw_env **out,
                 char *err, size_t errlen);
/* The same from the policies.yml text itself (read_policies_file + convert_yaml_map_to_json,
 * src/config.rs:419-453): YAML is converted to JSON, then built as above. A YAML error is a
 * KW_E_BOOTSTRAP. kw_yaml_to_json exposes the conversion (KW_E_PAYLOAD + message on error). */
int kw_env_build_yaml(const char *policies_yaml, size_t len, const kw_env_options *opts, kw_env **out,
                      char *err, size_t errlen);
int kw_yaml_to_json(const char *yaml, size_t len, char *buf, size_t cap, size_t *need);
/* Compiled-table blob (what rank 0 broadcasts over RCCL to the other GPUs). */
int kw_env_serialize(const kw_env *env, void *buf, size_t cap, size_t *need);
int kw_env_deserialize(const void *blob, size_t len, int device, kw_env **out, char *err, size_t errlen);
void kw_env_destroy(kw_env *env);

/* PolicyID::from_str (src/evaluation/policy_id.rs:29-47) + map lookup. Returns KW_OK and the
 * policy index, KW_E_INVALID_ID, or KW_E_NOT_FOUND. */
int kw_env_lookup(const kw_env *env, const char *policy_id, size_t len, int32_t *idx);
int kw_env_policy_count(const kw_env *env);
int kw_env_policy_id(const kw_env *env, int32_t idx, char *buf, size_t cap); /* PolicyID Display */
int kw_env_is_group(const kw_env *env, int32_t idx);
/* get_policy_mode / get_policy_allowed_to_mutate (evaluation_environment.rs:445-458) */
int kw_env_get_policy_mode(const kw_env *env, int32_t idx, int *mode);
int kw_env_get_policy_allowed_to_mutate(const kw_env *env, int32_t idx, int *allowed);
/* should_always_accept_requests_made_inside_of_namespace (evaluation_environment.rs:373-378) */
int kw_env_should_always_accept_requests_made_inside_of_namespace(const kw_env *env, const char *ns,
                                                                   size_t len);
/* policy_initialization_errors lookup (evaluation_environment.rs:569-571): 1 + message if set */
int kw_env_policy_initialization_error(const kw_env *env, int32_t idx, char *buf, size_t cap);
/* EvaluationEnvironment::validate_settings (evaluation_environment.rs:472-510): KW_OK, or
 * KW_E_INIT with the message (groups: expression validity, :496-506). */
int kw_env_validate_settings(const kw_env *env, int32_t idx, char *buf, size_t cap);
/* Diagnostic: does `s` match pattern `pat` (kind 0 literal, 1 glob, 2 regex) under the engine's
 * compiled-automaton semantics? 1/0, or -1 on a pattern syntax error. */
int kw_pattern_match(int kind, const char *pat, const char *s, size_t len);
/* The same for n subjects with one compilation: out[i] = 1/0; returns KW_OK, or -1 on a syntax
 * error. A pattern whose DFA exceeds the state budget runs as its NFA (kwdev.hpp DevNfa);
 * kind | KW_PATTERN_FORCE_NFA runs the NFA form whatever its DFA size (tests: DFA == NFA). */
#define KW_PATTERN_FORCE_NFA 0x100
int kw_pattern_match_many(int kind, const char *pat, const char *const *subjects, const size_t *lens, size_t n,
                          int32_t *out);
/* Diagnostics over the compiled classifiers (tests): the distinct patterns of request column `col`
 * (kwdev.hpp Col; kind 0 literal, 1 glob, 2 regex), and the ids of the patterns string `s` matches
 * through the blob's tables (the tables the kernels run). For COL_LV, `key` is the label key and
 * the result is restricted to the regexes constrained on it. kw_env_classify returns the number of
 * matched ids (writing at most `cap`), or -1. */
int kw_env_pattern_count(const kw_env *env, int col);
int kw_env_pattern(const kw_env *env, int col, int idx, int *kind, char *buf, size_t cap);
int kw_env_classify(const kw_env *env, int col, const char *key, size_t klen, const char *s, size_t len,
                    uint32_t *pats, int cap);

/* ---------------------------------------------------------------------------------------------
 * Request batches: the micro-batch handed over by the HTTP front (replaces the one
 * spawn_blocking task per request of acquire_semaphore_and_evaluate, handlers.rs:256-286).
 * ------------------------------------------------------------------------------------------- */
typedef struct kw_batch kw_batch;

/* Flatten n JSON documents (AdmissionReview {"request": AdmissionRequest} or RawReview
 * {"request": Value}) into SoA columns. A document that does not deserialize returns
 * KW_E_PAYLOAD with its row in *bad_row (the 422 of JsonExtractor, handlers.rs:29-39). */
int kw_batch_from_json(const char *const *docs, const size_t *lens, size_t n, int doc_kind,
                       kw_batch **out, int64_t *bad_row, char *err, size_t errlen);
/* Copy a caller-built SoA into a batch (the caller keeps ownership of its arrays). */
int kw_batch_from_soa(const kw_soa *soa, kw_batch **out);
/* Host view of the batch's columns (valid until kw_batch_destroy). */
int kw_batch_view(const kw_batch *b, kw_soa *view);
/* Upload the columns to HBM of `device` (synchronous; the bench times kernels with inputs resident).
 * Device memory and the pinned host staging come from per-device caching pools (returned when the
 * batch is destroyed), so a front that uploads thousands of micro-batches per second does not
 * allocate per batch. */
int kw_batch_to_device(kw_batch *b, int device);
/* The same, asynchronous on the caller's hipStream_t `stream` (which later passes of this batch use
 * by default); the upload completes in stream order. */
int kw_batch_to_device_async(kw_batch *b, int device, void *stream);
/* A non-blocking hipStream_t on `device` for callers without HIP headers (the HTTP front). */
int kw_stream_create(int device, void **stream);
void kw_stream_destroy(void *stream);
void kw_batch_destroy(kw_batch *b);

/* Diagnostic (test infrastructure, never called by kw_validate_*): evaluate the batch's rows
 * against the policy list on the HOST through the same slot compiler the device uses and the
 * sequential form of its first-violation walks (slots.hpp walk_*), with the column automata of the
 * blob. Lets the CPU test suite check the slot compiler against the oracle without a GPU.
 * out: [row][npol] verdict words. No reference counterpart (diagnostic only). */
int kw_debug_host_walk(const kw_env *env, const kw_batch *b, const int32_t *policies, uint32_t npol,
                       int origin, uint32_t *out);

/* Diagnostic (tests): plan an all-pairs pass over the batch's host columns without launching it.
 * out[0..8): LDS bytes per workgroup, launches, slot-plan chunks, classifiers staged in LDS (1) or
 * read from global memory (0), requests per tile, container / capability / label capacities (of the
 * first region). cap >= 16 adds out[8..16): regions (1, or 2 for a light / heavy split batch), the
 * light region's rows, the first region's grid, the heavy region's LDS bytes, requests per tile,
 * container capacity and grid, and a bit per region launched as the container wave-scan kernel. */
int kw_debug_plan(const kw_env *env, kw_batch *b, const int32_t *policies, uint32_t npol, int origin, uint32_t *out,
                  int cap);

/* Diagnostic (tests): the staging copy jobs of the tile kernel for an all-pairs pass planned over the
 * batch's host columns (nothing launched), with every tile descriptor and the span the kernel's own
 * span function gives each job in it. out (u32 words): regions; then per region
 *   8 words: requests per tile, jobs, descriptors, overflow requests, first and end row, LDS bytes,
 *            the light region's rows (0: batch order);
 *   20 words: LDS offsets of the staged request flags, container / label offsets, container flags,
 *            added / dropped capability offsets, then of each string column's offsets [7] and bytes [7]
 *            (0: not staged);
 *   per job 4 words: column (0-5 the arrays above in that order, 6 + 2m / 7 + 2m string column m's
 *            offsets / bytes), LDS destination, bytes per piece (4 or 16), the job's code;
 *   per descriptor 32 descriptor words, then per job 3 words: byte offset into the column (low,
 *            high) and pieces to copy;
 *   the overflow requests' rows.
 * *needed: the words of the whole record; KW_E_NOSPACE when cap is smaller (out untouched). */
int kw_debug_copy_jobs(const kw_env *env, kw_batch *b, const int32_t *policies, uint32_t npol, int origin,
                       uint32_t *out, size_t cap, size_t *needed);

/* Diagnostic (tests): the tile descriptors a resident all-pairs pass would upload, planned over the
 * batch's host columns (nothing launched), cut per tile at the least estimated cost per row
 * (KW_TILE_CUT), in row order. out (u32 words): regions, overflow requests; then per region
 *   10 words: requests per tile, container / capability / label capacity, grid, XCDs the grid's
 *            workgroups spread over (nx), schedule (0 strided, 1 dynamic), descriptors, first and end row;
 *   7 + 7 words: per string column whether it is staged, and its byte capacity;
 *   per descriptor, in array order, 34 words: the 32 descriptor words (first request at words 24-25,
 *            requests 26, fits 23; entity ranges 0-7) and the estimated cost in wave-cycles (low, high;
 *            0 for a descriptor queued for the overflow kernels);
 * then the overflow requests' rows. Rows are device rows (kw_debug_reorder).
 * *needed: the words of the whole record; KW_E_NOSPACE when cap is smaller (out untouched). */
int kw_debug_tile_descs(const kw_env *env, kw_batch *b, const int32_t *policies, uint32_t npol, int origin,
                        uint32_t *out, size_t cap, size_t *needed);

/* Diagnostic (tests): the planner's estimated cost in wave-cycles of a tile with these item counts,
 * for a launch of the family set `feat` (bits: 1 image, 2 label, 4 container, 8 group) that classifies
 * the string columns `need` (bit per column: 0 namespace, 1 image, 2 AppArmor, 3 / 4 added / dropped
 * capabilities, 5 / 6 label keys / values). */
uint64_t kw_debug_tile_cost(uint32_t feat, uint32_t need, uint32_t requests, uint32_t labels, uint32_t containers,
                            uint32_t capabilities);

/* Diagnostic (tests): the tile schedule's index arithmetic as the kernel and the planner share it,
 * for `workgroup` of a launch of `grid` workgroups over ndesc descriptors. out[0..7): XCDs in use, the
 * workgroup's XCD, its slot in that XCD, the XCD's workgroups, the XCD's descriptor range [lo, hi),
 * and the descriptor the slot runs as its `tile`-th tile on the strided schedule (one only while < hi). */
int kw_debug_tile_slot(uint64_t ndesc, uint32_t grid, uint32_t workgroup, uint32_t tile, uint64_t *out);

/* Diagnostic (tests): the counter schedule with `rounds` static rounds (a slot's first `rounds` tiles
 * strided, the rest of its XCD's range drawn from the XCD's counter), for `workgroup` as above.
 * out[0..7): the XCD's first descriptor, the workgroup's slot, the XCD's workgroups (its static tile k
 * is the descriptor lo + slot + k * workgroups), how many of the slot's static tiles exist, the XCD's
 * counter-drawn tail [tail_lo, hi), and the launch's whole rounds q (the least over its XCDs of the
 * rounds in which every slot has a tile). */
int kw_debug_sched_tail(uint64_t ndesc, uint32_t grid, uint32_t workgroup, uint32_t rounds, uint64_t *out);

/* Diagnostic (tests): the static rounds a launch of ndesc descriptors over `grid` workgroups is handed
 * under the current KW_SCHED / KW_SCHED_TAIL (*rounds; -1: the strided schedule, no counter).
 * dynamic: whether the launch's plan chose the dynamic schedule (kw_debug_tile_descs reports it). */
int kw_debug_sched_rounds(uint64_t ndesc, uint32_t grid, int dynamic, int *rounds);

/* Diagnostic (tests): the tile-kernel launches of the batch's last resident pass (kw_validate_batch,
 * kw_validate_rows), three words each: the workgroups launched (the planned grid clamped to what the
 * device holds at once), the launch's descriptors, and its static rounds (-1: strided, no counter).
 * *needed: words; KW_E_NOSPACE when cap is smaller; KW_E_ARG for a batch that is not resident. */
int kw_debug_last_launches(const kw_batch *b, int64_t *out, size_t cap, size_t *needed);

/* Diagnostic (tests): beside kw_debug_last_launches, the tile kernel each of those launches took, one
 * word each: 0 the generic kernel of the launch's family set, 1 the production-shape one (DESIGN.md
 * §5). *needed: words; KW_E_NOSPACE when cap is smaller; KW_E_ARG for a batch that is not resident. */
int kw_debug_last_kernels(const kw_batch *b, uint32_t *out, size_t cap, size_t *needed);

/* Diagnostic (tests): whether a tile launch of this shape qualifies for a production-shape kernel
 * (1) or takes the generic one (0) — the launch's own predicate over a launch record made of these
 * values. feat: the family bits of kw_debug_tile_cost, 16 NFA elements, 32 predecessor ranges by wave
 * scan; debug: the KW_TILE_DEBUG bits; nchunk: chunks of the launch; ncols / vec4: the first chunk's
 * verdict columns and whether they are stored 16 bytes at a time; timing: the phase clocks run. */
int kw_debug_prod_shape(uint32_t feat, int lds_tables, uint32_t debug, uint32_t nchunk, int rows_mode, int prefetch,
                        uint32_t ncols, int vec4, int timing);

/* Diagnostic (tests): the kernel (as kw_debug_last_kernels) each tile launch of a resident all-pairs
 * pass would take under the current settings, planned over the batch's host columns (nothing
 * launched), in launch order. *needed: words; KW_E_NOSPACE when cap is smaller (out untouched). */
int kw_debug_plan_kernels(const kw_env *env, kw_batch *b, const int32_t *policies, uint32_t npol, int origin,
                          uint32_t *out, size_t cap, size_t *needed);

/* Diagnostic (tests): beside kw_debug_last_launches, the variant each of those launches asked the tile
 * kernel's dispatch for, recorded where the launch is made, one word each: bits 0-5 the launch's
 * family and flag bits (the family bits of kw_debug_tile_cost, 16 NFA elements, 32 predecessor ranges
 * by wave scan), KW_VARIANT_LDS_TABLES, KW_VARIANT_TIMING (the phase clocks run), KW_VARIANT_PROD (the
 * production shape). *needed: words; KW_E_NOSPACE when cap is smaller; KW_E_ARG for a batch that is
 * not resident. */
#define KW_VARIANT_FEAT 0x3fu
#define KW_VARIANT_LDS_TABLES 0x100u
#define KW_VARIANT_TIMING 0x200u
#define KW_VARIANT_PROD 0x400u
int kw_debug_last_variants(const kw_batch *b, uint32_t *out, size_t cap, size_t *needed);

/* Diagnostic (tests): the variant (as kw_debug_last_variants) each tile launch of a resident all-pairs
 * pass would ask for under the current settings, planned over the batch's host columns (nothing
 * launched, no device needed), in launch order. *needed: words; KW_E_NOSPACE when cap is smaller. */
int kw_debug_plan_variants(const kw_env *env, kw_batch *b, const int32_t *policies, uint32_t npol, int origin,
                           uint32_t *out, size_t cap, size_t *needed);

/* Diagnostic (tests): the instantiation of the tile kernel the dispatch resolves a requested variant
 * to, as a variant word: several requests share one instantiation (the phase clocks keep three family
 * sets with LDS tables and run every other set on the every-family kernel; an NFA element takes the
 * every-family kernel). The dispatch itself picks the kernel by this function. */
uint32_t kw_debug_resolve_variant(uint32_t variant);

/* Diagnostic (tests): the device-row order kw_batch_to_device gives this batch — the light / heavy
 * split (rows with more than 5 containers after the others when they are 1-50 % of
 * a batch of >= 2^18 rows and hold >= 30 % of its containers; KW_SPLIT=0 / 1 never / always) — as a
 * new host batch *out in that order. *split: the light region's rows (0: not split, *out in batch
 * order); perm[d] (cap >= rows) the batch row at device row d. */
int kw_debug_reorder(const kw_batch *b, uint64_t *perm, size_t cap, uint64_t *split, kw_batch **out);

/* ---------------------------------------------------------------------------------------------
 * The hot path: EvaluationEnvironment::validate + service::evaluate constraints, batched.
 * Evaluates every row against each of the npol policies (indices from kw_env_lookup) on the GPU;
 * verdict words are laid out row-major [row][npol]. Runs asynchronously on `stream` (a
 * hipStream_t of the batch's device; NULL = the batch's own stream) into the batch's device
 * verdict buffer; kw_batch_verdicts copies them to the host, synchronising with that stream. A pass
 * on another stream than the batch's previous pass first waits for the previous one.
 * ------------------------------------------------------------------------------------------- */
int kw_validate_batch(const kw_env *env, kw_batch *b, const int32_t *policies, uint32_t npol,
                      int origin, void *stream);
/* Micro-batch form: row r is evaluated against row_policy[r] only (one verdict per row), the
 * shape of many concurrent /validate/{policy_id} calls. */
int kw_validate_rows(const kw_env *env, kw_batch *b, const int32_t *row_policy, int origin,
                     void *stream);
int kw_batch_verdicts(kw_batch *b, uint32_t *host_out, size_t count);
/* Bulk form for callers that hand over host columns and want host verdicts (SURVEY §8(d) timing
 * mode 2): uploads the batch to `device`, evaluates every row against the npol policies and writes
 * the [row][npol] verdict words to host `out` (count = rows x npol). The batch is cut into chunks of
 * about chunk_rows rows (0: 262144) whose upload, evaluation and read-back overlap on three streams;
 * only the string columns the pass reads are uploaded (a later pass on the batch that needs others
 * returns KW_E_ARG until the batch is uploaded again). `out` may be pageable (read back through
 * pinned bounce blocks) or pinned (kw_host_alloc: direct DMA). Passes that need several launches,
 * overflow requests or wide side data run unchunked with the same result. Synchronous. Replaces,
 * for a bulk caller, the per-request loop of acquire_semaphore_and_evaluate (handlers.rs:256-286). */
int kw_validate_host(const kw_env *env, kw_batch *b, const int32_t *policies, uint32_t npol, int origin,
                     int device, uint32_t *out, size_t count, uint32_t chunk_rows);
/* The packed verdict form of a pass of rows x npol: lossless, for bulk callers whose read-back is
 * the longer direction. A word without a violation depends only on its column (the
 * policy's mode and allowedToMutate, the origin) and on whether the response mutated or the request
 * was bypassed, so each (row, column) is a 2-bit code into a three-word dictionary per column, and
 * only the other words are stored. With G = ceil(npol / 64) column groups, all arrays caller-owned:
 *   dict     u32[npol][3]: the column's word for an accepted response, for an accepted and mutated
 *            one, and for a bypassed request (a column whose word is the same whatever the request
 *            holds that word first). A fixed function of (env, policies, origin).
 *   planes   u64[rows][G][2]: bit c of planes[r][g][0] / [1] is the low / high bit of the code of
 *            column 64 g + c. Codes 0-2: the word is dict[col][code] (the lowest matching index);
 *            code 3: the word is an exception. Bits of columns >= npol are 0.
 *   exc_off  u32[rows + 1]: exc_off[r] is the index in exc of row r's first exception, exc_off[rows]
 *            the total.
 *   exc      u32[exc_cap]: the exception words in (row, column) order: the word of (r, col) is
 *            exc[exc_off[r] + the number of code-3 columns of row r below col].
 *   exc_count (output) the exception words of the pass.
 * The same input gives the same bytes. No reference counterpart (an output form of the bulk entry). */
typedef struct kw_packed {
  uint64_t rows;
  uint32_t npol;
  uint64_t *planes;
  uint32_t *exc_off;
  uint32_t *exc;
  size_t exc_cap;
  uint32_t *dict;
  size_t exc_count;
} kw_packed;
/* kw_validate_host with the verdicts in the packed form: out->rows, npol, the five pointers and
 * exc_cap come from the caller (rows = the batch's, npol = the list's, else KW_E_ARG; so is a pass of
 * rows x npol >= 2^32). The device packs each chunk's words behind its kernels and only the planes,
 * the offsets and the exceptions are read back. Direct DMA when planes, exc_off and exc are all
 * page-locked (kw_host_alloc), else through pinned bounce blocks. When the exceptions exceed exc_cap
 * the pass still runs to its end: KW_E_NOSPACE with the need in out->exc_count, the arrays' contents
 * then unspecified. kw_batch_wide_arg and kw_batch_group_causes work after it as after
 * kw_validate_host. */
int kw_validate_host_packed(const kw_env *env, kw_batch *b, const int32_t *policies, uint32_t npol, int origin,
                            int device, kw_packed *out, uint32_t chunk_rows);
/* The verdict word of (row, col) of a packed pass; KW_E_ARG outside it. */
int kw_packed_word(const kw_packed *p, uint64_t row, uint32_t col, uint32_t *word);
/* Rows [row0, row1) of a packed pass as full words, out [row1 - row0][npol]. */
int kw_packed_unpack(const kw_packed *p, uint64_t row0, uint64_t row1, uint32_t *out);
/* Diagnostic (tests, documents): full words [rows][npol] into the packed form on the host, by the
 * reference encoder under the dictionary a device pass over (env, policies, origin) uses. out as
 * for kw_validate_host_packed (rows from the caller); KW_E_NOSPACE likewise. */
int kw_debug_pack_words(const kw_env *env, const int32_t *policies, uint32_t npol, int origin, const uint32_t *words,
                        uint64_t rows, kw_packed *out);
/* The summary form of a pass of rows x npol: lossy and fixed-size, for callers that count before
 * they read (an audit scan, a metrics exporter). Reduced on the device, so only the counters and, if
 * asked, two bits per pair cross PCIe instead of every word. With G = ceil(npol / 64) as in kw_packed,
 * all arrays caller-owned:
 *   col      u64[npol][KW_SUM_N]: col[c][k] counts column c's words. k 0-4: the words with the named
 *            bit set; 5-7: by F_STATUS value; KW_SUM_REASON + r: the words whose KW_REASON is r <= 15
 *            (index 16: no violation); KW_SUM_REASON_OTHER: any other reason. No product word has
 *            one; the KW_POISON_VERDICTS sentinel does, so a tile that was never evaluated shows up
 *            there. Indices 9-15 are zero.
 *   planes   u64[rows][G][2], or NULL for the counters alone: bit c of planes[r][g][0] is set when
 *            the word of column 64 g + c lacks KW_F_ALLOWED (the final answer is a reject), bit c of
 *            planes[r][g][1] when its KW_REASON is non-zero (the policy found something, whatever
 *            mode, bypass or constraints made of it): the pairs worth a message. A word counted
 *            in KW_SUM_REASON_OTHER sets both bits whatever its other bits say. Bits of columns
 *            >= npol are 0.
 * The same input gives the same bytes. The V_ALLOWED / V_MUTATED / INIT_ERROR counters are the
 * accepted / mutated / error counts kubewarden_policy_evaluations_total carries per policy
 * (src/metrics.rs:49-140) without the per-request attributes: the attribute sets with resource kind,
 * operation and namespace come from kw_batch_outcomes over kw_batch_attribute_groups
 * (kw_metrics_record_pass runs both), also on the device. */
enum {
  KW_SUM_F_ALLOWED = 0,
  KW_SUM_V_ALLOWED = 1,
  KW_SUM_V_MUTATED = 2,
  KW_SUM_F_PATCH = 3,
  KW_SUM_BYPASS = 4,
  KW_SUM_FST_VANILLA = 5,
  KW_SUM_FST_MUTATION_REFUSED = 6,
  KW_SUM_FST_INIT_ERROR = 7,
  KW_SUM_REASON_OTHER = 8, /* 9..15: zero */
  KW_SUM_REASON = 16,      /* + kw_reason, 0..15 */
  KW_SUM_N = 32
};
typedef struct kw_summary {
  uint64_t rows;
  uint32_t npol;
  uint64_t *col;    /* u64[npol][KW_SUM_N] */
  uint64_t *planes; /* u64[rows][G][2], or NULL: counters only */
} kw_summary;
/* The summary of the batch's last device pass (kw_validate_batch, kw_validate_rows or a bulk pass),
 * reduced in place on the device; synchronises with the pass's stream as kw_batch_verdicts does and
 * reads back only col and, if asked, the planes (in batch-row order). out->rows / npol must equal the
 * pass's, else KW_E_ARG (so is a batch without a pass); a kw_validate_rows pass is one column. */
int kw_batch_summary(kw_batch *b, kw_summary *out);
/* kw_validate_host with the summary as its only output: each chunk is reduced on the device behind
 * its kernels, its planes go out while the next chunk runs (direct DMA into page-locked planes, else
 * through pinned bounce blocks), the totals after the last chunk. out->rows = the batch's, npol = the
 * list's, else KW_E_ARG. The verdict words stay on the device: kw_batch_verdict_rows,
 * kw_batch_verdicts and kw_batch_summary work on the pass afterwards. */
int kw_validate_host_summary(const kw_env *env, kw_batch *b, const int32_t *policies, uint32_t npol, int origin,
                             int device, kw_summary *out, uint32_t chunk_rows);
/* The full words of n chosen batch rows of the last pass, out[n][row_words] (row_words: npol, or 1
 * after kw_validate_rows), gathered on the device and read back in one copy; any order, repeats
 * allowed. Loads the pass's side data as kw_batch_verdicts does, so kw_batch_wide_arg,
 * kw_batch_group_causes and the formatters work on the fetched words. A row >= the pass's rows gives
 * KW_E_ARG; n = 0 is KW_OK. The audit flow: summary, the rows whose plane 1 is non-zero, their words,
 * messages. */
int kw_batch_verdict_rows(kw_batch *b, const uint64_t *rows, size_t n, uint32_t *out);
/* The shape of the batch's last device pass, as kw_batch_summary and kw_batch_verdict_rows see it:
 * its rows and its verdict words per row (npol, or 1 after kw_validate_rows). A caller sizes the
 * output of kw_batch_verdict_rows by it. KW_E_ARG for a batch without a pass. */
int kw_batch_last_pass(const kw_batch *b, uint64_t *rows, uint32_t *row_words);
/* Diagnostic (tests, documents): full words [rows][npol] into the summary form on the host, by the
 * reference reducer. */
int kw_debug_summarize_words(const uint32_t *words, uint64_t rows, uint32_t npol, kw_summary *out);
/* The outcome of a verdict word: everything the attribute sets of kubewarden_policy_evaluations_total
 * (src/metrics.rs:49-140) take from it. KW_OUT_INIT_ERROR for a word whose F_STATUS is
 * KW_FST_INIT_ERROR (PolicyInitializationError, the counter only); else accepted | mutated << 1 |
 * error_code 500 << 2 of the vanilla response, where a bypassed request is accepted, not mutated and
 * carries no error code (service.rs:45-58), and the error code is that of a group expression that
 * failed (KW_R_GROUP_EXPR). Codes 0-7 are that bit pattern. */
enum {
  KW_OUT_REJECTED = 0,
  KW_OUT_ACCEPTED = 1,   /* bit */
  KW_OUT_MUTATED = 2,    /* bit */
  KW_OUT_ERROR_500 = 4,  /* bit */
  KW_OUT_INIT_ERROR = 8,
  KW_OUT_N = 9
};
/* The grouped outcome count of the batch's last device pass (kw_validate_batch, kw_validate_rows as
 * one column, or a bulk pass), counted on the device over the words where they lie: with npol the
 * pass's words per row (kw_batch_last_pass), out u64[ngroups][KW_OUT_N][npol] (caller-owned) gets in
 * out[g][k][c] the rows of group g whose word in column c has outcome k. row_group[rows] gives each
 * batch row's group id < ngroups (NULL: one group); with the ids of kw_batch_attribute_groups a
 * counter is one series of kubewarden_policy_evaluations_total (src/metrics.rs:49-140), with any
 * other ids, such as one per namespace, the pass / fail / mutated totals a policy report holds. Only
 * the row list goes to the device and only the table comes back; tables beyond the KW_OUTCOME_TABLE
 * budget (bytes, default 64 MB) are counted in consecutive group ranges. The same input gives the same
 * bytes. KW_E_ARG for an id >= ngroups, ngroups = 0 and a batch without a pass; a pass of zero rows
 * gives an all-zero table. */
int kw_batch_outcomes(kw_batch *b, const uint32_t *row_group, uint32_t ngroups, uint64_t *out);
/* Diagnostic (tests, documents): the same table from full words [rows][npol] on the host, by the
 * reference reducer (src/metrics.rs:49-140 as above). */
int kw_debug_outcome_words(const uint32_t *words, uint64_t rows, uint32_t npol, const uint32_t *row_group,
                           uint32_t ngroups, uint64_t *out);
/* The dictionary of what the attribute sets (src/metrics.rs:49-140) read from a row, host only: all
 * raw rows (KW_REQ_RAW) are one group; every other row is keyed by (request.requestKind.kind or "",
 * operation, whether it has a namespace, namespace), so a row without a namespace and one whose
 * namespace is "" differ. Ids are numbered by first appearance in batch order; row_group[rows] (or
 * NULL) gets each row's id, first_row[g] (cap entries, or NULL) the first row of group g, *ngroups
 * the count. KW_E_NOSPACE with *ngroups filled in when cap is smaller (row_group is still written).
 * The batch keeps the result: a second call does not rebuild it. */
int kw_batch_attribute_groups(const kw_batch *b, uint32_t *row_group, uint64_t *first_row, size_t cap,
                              uint32_t *ngroups);
/* The violation digest of a pass of rows x npol: its findings grouped by cause, for callers that want
 * to know what is wrong and how often before they format a single message (an audit scan over many
 * Pods). A finding is a pair (row, column) whose word has KW_REASON != 0. Its key is what the message
 * of the reason quotes from the request or the settings, apart from the container's name:
 *   KW_R_PRIVILEGED                      nothing
 *   KW_R_NAMESPACE                       the row's ns string
 *   KW_R_REG_NOT_ALLOWED..KW_R_IMG_REJECTED  the ctr_image string, as it stands in the column, of
 *                                        container ctr_off[row] + ARG
 *   KW_R_CAP_NOT_ALLOWED                 the cap_add string at capadd_off[ctr_off[row]] + ARG
 *   KW_R_APPARMOR                        ctr_apparmor of container ctr_off[row] + ARG
 *   KW_R_LABEL_DENIED                    lbl_key of label lbl_off[row] + ARG
 *   KW_R_LABEL_CONSTRAINT                that label's key and value, two strings whose lengths are part
 *                                        of the key: ("ab", "c") and ("a", "bc") differ
 *   any other reason (12-15, and values no product word has, such as the KW_POISON_VERDICTS
 *   sentinel's)                          the 16-bit ARG as a number
 * (an entity index the column does not hold, which no product word names, reads as ""). Two findings
 * are one group when their column, their reason, their KW_F_ALLOWED bit (a finding that was let
 * through does not mix with one that rejected) and their key, byte for byte, are equal. A finding
 * whose ARG is KW_ARG_WIDE belongs to no group when its reason takes an entity index (1, 3-11) or is
 * KW_R_GROUP: it is listed in `wide` as the pair index row * npol + col, for kw_batch_wide_arg /
 * kw_batch_group_causes. All arrays caller-owned:
 *   recs      kw_digest_rec[cap]: the groups ordered by (col, reason, first_row). first_row is the
 *             group's lowest batch row, word the verdict word of (first_row, col), so
 *             kw_format_response(row = first_row, ..., word) gives a representative message; count the
 *             group's findings. Two groups of one column never share a first_row: the order is total.
 *   wide      u64[wide_cap]: the wide findings' pair indices, ascending.
 *   n, nwide, findings (outputs): the groups, the wide findings, and all findings of the pass, the
 *             wide ones included: the counts of recs add up to findings - nwide.
 * When cap or wide_cap is too small: KW_E_NOSPACE with the exact n and nwide, the arrays' contents
 * then unspecified (as kw_validate_host_packed treats exc_cap). The same input gives the same bytes.
 * No reference counterpart (an output form of a pass, as the packed and the summary forms). */
typedef struct kw_digest_rec {
  uint32_t col;
  uint32_t word;
  uint64_t first_row;
  uint64_t count;
} kw_digest_rec;
typedef struct kw_digest {
  kw_digest_rec *recs;
  size_t cap;
  size_t n;
  uint64_t *wide;
  size_t wide_cap;
  size_t nwide;
  uint64_t findings;
} kw_digest;
/* The digest of the batch's last all-pairs device pass (kw_validate_batch or a bulk pass), reduced on
 * the device over the words where they lie and the string columns the pass read: the findings are
 * hashed into a table of KW_DIGEST_TABLE bytes (default 64 MB), a second launch compares every
 * finding's key bytes with its group's representative so that the result is exact whatever the hash
 * does, and only the records and the wide list come back. Synchronises with the pass's stream as
 * kw_batch_summary does. A group never spans columns: a pass with more groups than the table takes
 * is reduced in column ranges, halved until each fits; KW_E_NOSPACE with n = 0 only when the groups
 * of a single column do not fit (more than half of the table's 24-byte slots, a power of two, or, with
 * KW_DIGEST_HASH_BITS lowered, more colliding findings than the leftover list of 65536 holds).
 * KW_E_ARG after kw_validate_rows (its one column has a policy per row), for a batch without a pass,
 * for rows >= 2^32 and when a finding's key column is not resident (a bulk pass uploads only the
 * columns it reads, which are the ones its reasons quote). A pass without findings gives n = 0. */
int kw_batch_digest(kw_batch *b, kw_digest *out);
/* Diagnostic (tests, documents): the same digest from full words [rows][npol] (rows <= the batch's)
 * and the host batch, by the reference reducer: an ordered map over the exact keys, no hashing. */
int kw_debug_digest_words(const kw_batch *b, const uint32_t *words, uint64_t rows, uint32_t npol, kw_digest *out);
/* The key bytes of the finding `word` at batch row `row`, host only: *need bytes (written while they
 * fit in cap, else KW_E_NOSPACE). For KW_R_LABEL_CONSTRAINT the label's key is followed by its value
 * and *split is the key's length; otherwise *split = *need. A numeric or empty key has need 0. */
int kw_batch_finding_key(const kw_batch *b, uint64_t row, uint32_t word, char *buf, size_t cap, size_t *need,
                         size_t *split);
/* Diagnostic (tests): what the batch's last kw_batch_digest did. out[0..4): the column ranges that ran
 * to the end, the findings the verify launch handed to the host (leftovers), the table's slots, and
 * the ranges that were cut. KW_E_ARG for a batch that was never digested. */
int kw_debug_digest_stats(const kw_batch *b, uint64_t *out);
/* The drill-down of the digest: the members of the groups a caller names, for the step between
 * "what is wrong and how often" and the messages (tickets, labels, the per-resource entries of a
 * policy report). Record g of `groups` names the group of the finding at (groups[g].first_row,
 * groups[g].col): the pairs of that column with the same reason, the same KW_F_ALLOWED bit and a
 * byte-equal key (the rules of kw_digest above). Only col, word and first_row are read: count is
 * ignored, and first_row may be any member of the group, with word its word. All arrays caller-owned:
 *   off    u64[ngroups + 1], required when ngroups > 0: off[g] .. off[g + 1] bound group g's members
 *          in rows and words, in the order of the caller's list.
 *   rows   u64[cap]: the members' batch rows (never device rows, also for a split batch), ascending
 *          within a group; a group holds a row at most once (a group lives in one column and a pair
 *          has one word).
 *   words  u32[cap], or NULL for the rows only: the verdict word of (rows[i], the group's col), so
 *          kw_format_response(env, b, rows[i], policy of col, words[i], ...) gives each member's exact
 *          message with no further read-back.
 *   n (output): the members of all named groups together.
 * For the records of a digest of the same pass: off[g + 1] - off[g] = count, rows[off[g]] =
 * first_row, words[off[g]] = word. When n > cap: KW_E_NOSPACE with n and all of off exact, the
 * contents of rows and words then unspecified (as kw_digest treats cap). KW_E_ARG: col >= the pass's
 * columns or first_row >= its rows; a word that is not a finding, or is a wide finding (those are
 * listed in kw_digest.wide and belong to no group); a word that differs from the pass's word at
 * (first_row, col), as a record of another pass does; two records that name the same group; off NULL
 * with ngroups > 0; rows NULL with cap > 0. ngroups = 0 is KW_OK with n = 0. The same input gives the
 * same bytes. No reference counterpart (an output form of a pass, as the packed, the summary and the
 * digest forms). */
typedef struct kw_members {
  uint64_t *off;
  uint64_t *rows;
  uint32_t *words;
  size_t cap;
  size_t n;
} kw_members;
/* The members over the batch's last all-pairs device pass (kw_validate_batch or a bulk pass), found
 * on the device over the words where they lie, as kw_batch_digest reads them: the named groups go
 * into a selection table built on the host from the host batch's columns, one launch checks every
 * record's word against the pass, one walk over the words probes the table for each finding whose
 * (reason, allowed) class some named group of its column has and compares its key bytes with the
 * representative's, so the result is exact whatever the hash does; only the per-group counts and
 * the members come back, and the host orders them. Does not depend on KW_DIGEST_TABLE,
 * KW_DIGEST_HASH_BITS or KW_SPLIT, nor on whether kw_batch_digest ran. Synchronises with the pass's
 * stream as kw_batch_digest does. KW_E_ARG as above and, as for the digest, after kw_validate_rows,
 * for a batch without a pass, for rows >= 2^32 and when a record's key column is not resident. A
 * KW_E_ARG or KW_E_NOSPACE leaves the batch good for further calls. */
int kw_batch_digest_members(kw_batch *b, const kw_digest_rec *groups, size_t ngroups, kw_members *out);
/* Diagnostic (tests, documents): the same members from full words [rows][npol] (rows <= the batch's)
 * and the host batch, by the reference reducer: an ordered map over the exact keys, no hashing. */
int kw_debug_digest_members_words(const kw_batch *b, const uint32_t *words, uint64_t rows, uint32_t npol,
                                  const kw_digest_rec *groups, size_t ngroups, kw_members *out);
/* The last step of the audit flow on the device: the messages of chosen findings. The message of
 * item i, the pair (rows[i], cols[i]) of the batch's last all-pairs device pass, is the byte string
 * kw_format_response puts into status.message for a plain policy: the policy's own text for the
 * pass's word at that pair (its KW_REASON and KW_ARG), raw UTF-8 with no JSON escaping, whatever
 * mode, bypass or constraints made of the word (the digest counts a finding that was let through in
 * the same way). A word of reason 0, or of a reason no product word has, has the empty message.
 * `policies` [npol] is the policy list of that pass: the batch does not record the list of every
 * kind of pass, so it is the caller's contract, as the policy argument of kw_format_response is;
 * only its length is checked against the pass. All arrays caller-owned:
 *   off    u64[n + 1], required when n > 0: message i is text[off[i] .. off[i + 1]).
 *   text   cap bytes; page-locked memory (kw_host_alloc) is written by direct DMA, pageable memory
 *          through pinned bounce blocks.
 *   bytes  (output) off[n].
 *   words  u32[n] or NULL: the pass's word of each item.
 *   host   u64[host_cap]: the indices i, ascending, of the items the device does not render. They
 *          have a zero-length message here and are left to kw_format_response: reason
 *          KW_R_GROUP_EXPR (its text may be replaced by a data-dependent one), a word of reason 1-12
 *          whose ARG is KW_ARG_WIDE (its argument is in the pass's side data), and a word whose
 *          argument the request does not hold (no product word). nhost (output): their number.
 * Items are in the caller's order; any order and repeats are allowed; rows are batch rows, never
 * device rows, also for a split batch. When bytes > cap or nhost > host_cap: KW_E_NOSPACE with bytes,
 * nhost and all of off exact, text and host then unspecified (as kw_members treats cap). KW_E_ARG: a
 * row or col outside the pass; npol other than the pass's words per row; a batch without a pass; a
 * pass of kw_validate_rows; a policy index outside the env's visible policies; a message that quotes
 * a string column that is not resident; off NULL with n > 0; text NULL with cap > 0; host NULL with
 * host_cap > 0. n = 0 is KW_OK. The same input gives the same bytes. A KW_E_ARG or KW_E_NOSPACE
 * leaves the batch good for further calls. The container names, which no pass reads, are uploaded
 * from the host batch by the first call and kept until the batch is uploaded again or destroyed.
 * The items run in rounds of at most KW_MESSAGES_CHUNK; a round's lengths, their scan and the text
 * are three steps on the device, the text written through windows of KW_MESSAGES_WINDOW bytes. Synchronises
 * with the pass's stream. No reference counterpart (an output form of a pass). */
typedef struct kw_messages {
  uint64_t *off;
  char *text;
  size_t cap;
  size_t bytes;
  uint32_t *words;
  uint64_t *host;
  size_t host_cap, nhost;
} kw_messages;
int kw_batch_messages(kw_batch *b, const kw_env *env, const int32_t *policies, uint32_t npol,
                      const uint64_t *rows, const uint32_t *cols, size_t n, kw_messages *out);
/* Diagnostic (tests, documents): the same output on the host from full words [nrows][npol] (nrows <=
 * the batch's) and the host batch. how = 0: one policy_message call per item, the reference (an item
 * whose argument the request does not hold is listed in host instead of failing the call); how = 1:
 * the piece renderer the device runs (csrc/messages.hpp), over the host columns. */
int kw_debug_messages_words(const kw_env *env, const kw_batch *b, const int32_t *policies, uint32_t npol,
                            const uint32_t *words, uint64_t nrows, const uint64_t *rows,
                            const uint32_t *cols, size_t n, int how, kw_messages *out);
/* Diagnostic (tests): what the batch's last kw_batch_messages did. out[0..5): the rounds, the
 * staging windows written, the messages that spanned more than one window, the items listed for the
 * host, and whether that call uploaded the container names (1 / 0). KW_E_ARG for a batch that never
 * ran the call. */
int kw_debug_messages_stats(const kw_batch *b, uint64_t *out);
/* Where the audit flow ends: the whole AdmissionResponse bodies of chosen pairs, rendered on the
 * device. Response i is, byte for byte, what kw_format_response(env, b, rows[i], policies[cols[i]],
 * w, mv, ...) writes, w the pass's word at the pair and, for a group, mv[s] the pass's word at
 * (rows[i], c_s), c_s the first column with policies[c_s] equal to the group's member s: the uid echo,
 * `allowed`, status.message JSON-escaped, `code`, and a group's details.causes with the field and the
 * message of every rejecting member ("mutation is not allowed inside of policy group" for a member
 * that is allowed and mutated). Strings are escaped exactly as the host formatter escapes them: the
 * quote, the backslash, \n \r \t \b \f in two bytes, any other byte below 0x20 as \u00xx in lower-case
 * hex, every other byte unchanged (invalid UTF-8 included). The fields, the capacities, KW_E_NOSPACE
 * (bytes, nhost and all of off exact), the argument errors, any order and repeats of items, batch
 * rows for a split batch, page-locked or pageable `text`, the same bytes for the same input and
 * "leaves the batch good for further calls" are word for word kw_batch_messages' contract. The items
 * in `host` have a zero-length response here and are left to kw_format_response(_doc):
 *   every item for which kw_format_response answers an error instead of a response (KW_F_PATCH, an
 *   unregistered policy on the bypass path, a group with a broken member); reason KW_R_GROUP_EXPR; a
 *   word of reason 1-12 whose ARG is KW_ARG_WIDE; a group word whose ARG is KW_ARG_WIDE (more than 15
 *   members); a group with a member that is no column of the pass; a group with a cause whose own
 *   message is left to the host by these rules; an argument the request does not hold.
 * The uid column, like the container names, is uploaded from the host batch by the first call and
 * kept until the batch is uploaded again or destroyed. The items run in rounds of at most
 * KW_MESSAGES_CHUNK, the text through windows of KW_MESSAGES_WINDOW bytes. kw_batch_messages and its
 * bytes are unchanged by this call. Synchronises with the pass's stream. Replaces one
 * kw_format_response per pair (service::evaluate's response building). */
typedef struct kw_responses {   /* the fields of kw_messages, same meaning */
  uint64_t *off;
  char *text;
  size_t cap;
  size_t bytes;
  uint32_t *words;
  uint64_t *host;
  size_t host_cap, nhost;
} kw_responses;
int kw_batch_responses(kw_batch *b, const kw_env *env, const int32_t *policies, uint32_t npol,
                       const uint64_t *rows, const uint32_t *cols, size_t n, kw_responses *out);
/* Diagnostic (tests, documents): the same output on the host from full words [nrows][npol] (nrows <=
 * the batch's) and the host batch; the members' words are read from the same matrix. how = 0: one
 * format_response per item, the reference (an item it answers an error for is listed in host instead
 * of failing the call); how = 1: the part and piece renderer the device runs (csrc/responses.hpp),
 * over the host columns. */
int kw_debug_responses_words(const kw_env *env, const kw_batch *b, const int32_t *policies, uint32_t npol,
                             const uint32_t *words, uint64_t nrows, const uint64_t *rows,
                             const uint32_t *cols, size_t n, int how, kw_responses *out);
/* Diagnostic (tests): what the batch's last kw_batch_responses did. out[0..6): the rounds, the
 * staging windows written, the responses that spanned more than one window, the items listed for
 * the host, whether that call uploaded a side column (the uid column or the container names; 1 / 0),
 * and the pieces whose escaped length exceeded their raw length. KW_E_ARG for a batch that never ran
 * the call. */
int kw_debug_responses_stats(const kw_batch *b, uint64_t *out);

/* ---- accepted mutations: the JSONPatch of a pair, from columns ------------------------------------
 * The patch of a psp-capabilities policy needs the container's capability lists (columns already) and
 * the shape of the document around them. The batch keeps that shape in two host-side columns beside
 * kw_soa (whose layout is unchanged): per container a u32 KW_PS_PLACE(shape, index), index the item's
 * place in its own JSON array (containers, initContainers or ephemeralContainers; items that are no
 * objects count), and per request a u8 KW_PP_* naming the Pod-spec pointer. kw_batch_from_json fills
 * both; a batch made from a kw_soa holds "unknown" everywhere until kw_batch_set_patch_shape. */
enum kw_patch_shape {
  KW_PS_UNKNOWN = 0,
  KW_PS_NO_SC = 1,    /* securityContext is no object (absent, null, a string, ...) */
  KW_PS_NO_CAPS = 2,  /* securityContext is an object, capabilities is none */
  KW_PS_CAPS = 3,     /* capabilities is an object; plus KW_PS_ADD_ARRAY and / or KW_PS_DROP_ARRAY: */
  KW_PS_ADD_ARRAY = 1,  /*   `add` is an array  */
  KW_PS_DROP_ARRAY = 2, /*   `drop` is an array */
  KW_PS_MAX = 6
};
#define KW_PS_SHIFT 28
#define KW_PS_INDEX_MASK 0x0fffffffu
#define KW_PS_PLACE(shape, index) (((uint32_t)(shape) << KW_PS_SHIFT) | ((uint32_t)(index) & KW_PS_INDEX_MASK))
#define KW_PS_SHAPE(place) ((uint32_t)(place) >> KW_PS_SHIFT)
#define KW_PS_INDEX(place) ((uint32_t)(place) & KW_PS_INDEX_MASK)
enum kw_patch_pointer {
  KW_PP_UNKNOWN = 0,
  KW_PP_NONE = 1,      /* the object has no Pod spec: the patch is [] */
  KW_PP_POD = 2,       /* /spec */
  KW_PP_TEMPLATE = 3,  /* /spec/template/spec */
  KW_PP_CRONJOB = 4    /* /spec/jobTemplate/spec/template/spec */
};
/* Sets both columns. n_containers and n_requests must be the batch's, every shape <= KW_PS_MAX and
 * every pointer <= KW_PP_CRONJOB, else KW_E_ARG and the batch is unchanged. Before or after
 * kw_batch_to_device: a device copy of the columns is dropped and uploaded again on next use. */
int kw_batch_set_patch_shape(kw_batch *b, const uint32_t *ctr_place, uint64_t n_containers,
                             const uint8_t *req_place, uint64_t n_requests);
/* Reads both columns back (either pointer may be NULL); the sizes must be the batch's. */
int kw_batch_patch_shape(const kw_batch *b, uint32_t *ctr_place, uint64_t n_containers, uint8_t *req_place,
                         uint64_t n_requests);
enum kw_patch_form {
  KW_PATCH_OPS = 0,      /* the RFC 6902 ops: [{"op":"add","path":...,"value":...},...] */
  KW_PATCH_RESPONSE = 1  /* {"uid":U,"allowed":true,"patchType":"JSONPatch","patch":"<base64 of the ops>"} */
};
/* One pair's patch from the host columns, without the document: byte for byte the ops
 * capabilities_patch cuts from the document (form KW_PATCH_OPS), or the response
 * kw_format_response_doc writes (KW_PATCH_RESPONSE). buf / cap / need as kw_format_response. KW_E_ARG,
 * with a message in buf that names what is missing, where kw_batch_patches lists the item for the
 * host: a verdict without KW_F_PATCH, a policy that is no psp-capabilities policy (where
 * kw_format_response_doc answers KW_E_ENGINE), a request whose pointer or a container whose shape is
 * unknown. */
int kw_format_patch(const kw_env *env, const kw_batch *b, uint64_t row, int32_t policy, uint32_t verdict, int form,
                    char *buf, size_t cap, size_t *need);
/* The patches of chosen pairs of the last all-pairs device pass, rendered on the device: item i is
 * what kw_format_patch(env, b, rows[i], policies[cols[i]], w, form, ...) writes, w the pass's word at
 * the pair. The fields, the capacities, KW_E_NOSPACE (bytes, nhost and all of off exact), the
 * argument errors (a rows-mode pass, a policy list of another length, a row or a column outside the
 * pass: KW_E_ARG), any order and repeats of items, batch rows for a split batch, page-locked or
 * pageable `text`, the same bytes for the same input and "leaves the batch good for further calls"
 * are word for word kw_batch_responses' contract. The items in `host` have a zero length here:
 *   an item whose word has no KW_F_PATCH; an item whose column is no psp-capabilities policy; an item
 *   whose request's pointer is KW_PP_UNKNOWN; an item one of whose containers has shape
 *   KW_PS_UNKNOWN; an item whose row or container range the columns do not hold.
 * So the host list of kw_batch_responses can be handed to this call as it stands: its KW_F_PATCH
 * items are rendered, the others listed again. The two shape columns, like the uid column, are
 * uploaded from the host batch by the first call (in device-row order for a split batch) and kept
 * until the batch is uploaded again, the shape is set again or the batch is destroyed. A capability
 * column that the pass did not make resident is KW_E_ARG. Rounds of KW_MESSAGES_CHUNK, windows of
 * KW_MESSAGES_WINDOW bytes. Synchronises with the pass's stream. */
int kw_batch_patches(kw_batch *b, const kw_env *env, const int32_t *policies, uint32_t npol,
                     const uint64_t *rows, const uint32_t *cols, size_t n, int form, kw_responses *out);
/* Diagnostic (tests, documents): the same output on the host from full words [nrows][npol] and the
 * host batch. how = 0: one kw_format_patch per item, the reference (an item it answers an error for
 * is listed in host); how = 1: the renderer the device runs (csrc/patches.hpp), in the device's
 * rounds and windows, over the host columns. */
int kw_debug_patches_words(const kw_env *env, const kw_batch *b, const int32_t *policies, uint32_t npol,
                           const uint32_t *words, uint64_t nrows, const uint64_t *rows, const uint32_t *cols,
                           size_t n, int form, int how, kw_responses *out);
/* Diagnostic (tests): what the batch's last kw_batch_patches did. out[0..5): the rounds, the staging
 * windows written, the items that spanned more than one window, the items listed for the host,
 * whether that call uploaded a side column (the shapes or the uids; 1 / 0). KW_E_ARG for a batch that
 * never ran the call. */
int kw_debug_patches_stats(const kw_batch *b, uint64_t *out);
/* Page-lock the batch's large host column arrays in place (hipHostRegister; undone by
 * kw_batch_destroy) so kw_validate_host sends them to the device by DMA from where they lie instead
 * of through the pinned staging its host workers fill. For a caller that runs several bulk passes
 * over one batch, or that builds batches once and keeps them; registering costs about as much as one
 * staging fill. Arrays under 64 KiB, and any the runtime declines, stay staged. No reference
 * counterpart (a host-memory option of the bulk entry point). */
int kw_batch_pin_host(kw_batch *b, int device);
/* Pinned (page-locked) host memory for verdict buffers a caller keeps (direct DMA), and its release. */
int kw_host_alloc(int device, size_t bytes, void **out);
void kw_host_free(void *p);
/* The full argument of a verdict word whose ARG is KW_ARG_WIDE, for (row, policy) of the last pass
 * whose verdicts were copied (kw_batch_verdicts). KW_E_NOT_FOUND when the pass recorded none. */
int kw_batch_wide_arg(const kw_batch *b, uint64_t row, int32_t policy, uint64_t *value);
/* The causes of a policy-group rejection (REASON KW_R_GROUP) of the last copied pass as a member
 * bitset (bit s: the group's member s, settings order, was called by the expression and rejected;
 * evaluation_environment.rs:979-1042): from the word's ARG, or the pass's side data for groups with
 * more than 15 members (any number of members: `words` holds ceil(members / 64) u64, `needed` gets
 * that count; KW_E_NOSPACE when nwords is smaller). Replaces the causes of
 * PolicyGroupEvaluator::validate's AdmissionResponse (upstream policy-evaluator). */
int kw_batch_group_causes(const kw_batch *b, uint64_t row, int32_t policy, uint32_t verdict, uint64_t *words,
                          size_t nwords, size_t *needed);

typedef struct kw_timing {
  double classify_ms;   /* 0: classification is fused into the evaluation kernel */
  double evaluate_ms;   /* avg device time of one whole validate pass (every launch of it) */
  double total_ms;      /* avg device time of one whole validate pass */
  double classify_bytes;/* 0 */
  double evaluate_bytes;/* algorithmic bytes per pass */
} kw_timing;
/* Time `reps` back-to-back validate passes with HIP events on the launch stream. */
int kw_validate_timed(const kw_env *env, kw_batch *b, const int32_t *policies, uint32_t npol,
                      int origin, int warmup, int reps, kw_timing *out);

/* ---------------------------------------------------------------------------------------------
 * Responses. Build the AdmissionResponse JSON of one (row, policy) from its verdict word, exactly
 * as service::evaluate would return it (uid echo, status message/code, group causes).
 * member_verdicts: verdict words of the group's members for this row (settings order) or NULL
 * for a non-group policy.
 * ------------------------------------------------------------------------------------------- */
int kw_format_response(const kw_env *env, const kw_batch *b, uint64_t row, int32_t policy,
                       uint32_t verdict, const uint32_t *member_verdicts, char *buf, size_t cap,
                       size_t *need);
/* The same with the row's original document (doc_kind KW_DOC_*), which an accepted mutation
 * (KW_F_PATCH) needs: the response then carries patchType "JSONPatch" and the base64 RFC 6902
 * patch that adds the psp-capabilities policy's missing required drops / default adds to every
 * container (the mutated_object of the guest, returned as a patch by policy-evaluator [upstream];
 * DESIGN.md §2). kw_format_response answers KW_E_ARG for such a verdict. */
int kw_format_response_doc(const kw_env *env, const kw_batch *b, uint64_t row, int32_t policy,
                           uint32_t verdict, const uint32_t *member_verdicts, const char *doc,
                           size_t doc_len, int doc_kind, char *buf, size_t cap, size_t *need);
/* Group member policy indices (settings order) of a group; returns the count. */
int kw_env_group_members(const kw_env *env, int32_t group, int32_t *out, int cap);

/* service::evaluate for one request, end to end (service.rs:30-152): PolicyID parse, namespace
 * bypass, validate on the device, constraints, response JSON. Returns KW_OK with the response,
 * or the EvaluationError code (with Display message in buf) that the handler maps to HTTP. */
int kw_evaluate(const kw_env *env, const char *policy_id, const char *doc, size_t doc_len,
                int doc_kind, int origin, char *buf, size_t cap, size_t *need);

/* validation_response_with_constraints (service.rs:160-208) on a vanilla response given as
 * flags, for the reference's own truth-table tests. in/out flags: bit0 allowed, bit1 has patch,
 * bit2 has status. Returns the F_STATUS kind of the result. */
int kw_service_constraints(uint32_t vanilla_flags, int mode, int allowed_to_mutate,
                           uint32_t *out_flags);

/* ---------------------------------------------------------------------------------------------
 * Metrics (src/metrics.rs:49-140, src/metrics/policy_evaluations_{total,latency}.rs; recorded by
 * service::evaluate, src/api/service.rs:40-71, :78-84, :118-150). A kw_metrics aggregates the
 * counter kubewarden_policy_evaluations_total and the u64 histogram
 * kubewarden_policy_evaluation_latency_milliseconds with the reference's attribute sets:
 *   AdmissionRequest: policy_name, policy_mode, resource_kind (requestKind.kind),
 *     resource_request_operation, accepted, mutated, request_origin[, resource_namespace][, error_code]
 *   Raw: policy_name, policy_mode, accepted, mutated[, error_code]
 *   initialization error (counter only): policy_name, initialization_error
 * accepted / mutated / error_code are the vanilla response's (before constraints); a namespace
 * bypass counts as accepted, not mutated. Thread-safe; kept off the device path.
 * ------------------------------------------------------------------------------------------- */
typedef struct kw_metrics kw_metrics;
kw_metrics *kw_metrics_create(void);
void kw_metrics_destroy(kw_metrics *m);
/* Record n evaluated (row, policy) pairs of one validate pass: rows[i] of batch b against
 * policies[i], with their final verdict words and the latency from arrival to verdict in ms. Only
 * the policies the requests addressed are recorded (not a group's member rows). */
int kw_metrics_record(kw_metrics *m, const kw_env *env, const kw_batch *b, const uint64_t *rows,
                      const int32_t *policies, const uint32_t *verdicts, const uint64_t *latency_ms,
                      size_t n, int origin);
/* What kw_metrics_record would add for every (row, policy) pair of a pass that all share latency_ms,
 * from the pass's grouped outcome count instead of its words (src/metrics.rs:49-140): counts
 * u64[ngroups][KW_OUT_N][npol] as kw_batch_outcomes gives it over the groups of
 * kw_batch_attribute_groups, first_row[g] a row of group g (the attributes are read from it). A
 * counter n adds n to its series of kubewarden_policy_evaluations_total and, unless its outcome is
 * KW_OUT_INIT_ERROR, n observations of latency_ms to the histogram. The label set is built once per
 * non-zero counter, under one lock for the call. A policy index outside the visible policies is
 * skipped, as kw_metrics_record skips it; a first_row outside the batch is KW_E_ARG. Host only. */
int kw_metrics_add_outcomes(kw_metrics *m, const kw_env *env, const kw_batch *b, const int32_t *policies,
                            uint32_t npol, int origin, uint64_t latency_ms, const uint64_t *first_row,
                            uint32_t ngroups, const uint64_t *counts);
/* The metrics of the batch's last all-pairs device pass over `policies` (src/metrics.rs:49-140):
 * kw_batch_attribute_groups, kw_batch_outcomes, kw_metrics_add_outcomes. Only the table crosses
 * PCIe. KW_E_ARG when npol is not the pass's words per row, after a kw_validate_rows pass (its one
 * column has a policy per row) and for a batch without a pass. */
int kw_metrics_record_pass(kw_metrics *m, const kw_env *env, kw_batch *b, const int32_t *policies, uint32_t npol,
                           int origin, uint64_t latency_ms);
/* Prometheus text exposition (format 0.0.4) of everything recorded so far. */
int kw_metrics_render(const kw_metrics *m, char *buf, size_t cap, size_t *need);
void kw_metrics_reset(kw_metrics *m);

const char *kw_version(void);

#ifdef __cplusplus
}
#endif
#endif /* KWGPU_H */
