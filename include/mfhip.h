/*
 * mfhip.h -- C ABI of libmfhip.so, the MI355X-native DSGD / online-MF hot path.
 *
 * The reference (Mallik-G/large-scale-recommendation, Scala 2.11) runs this path on
 * Flink/Spark; a Scala shim binds these entry points over JNI.
 * Each entry point names the reference interface it replaces (file:line, paths as in
 * fl/mf = flink-adaptive-recom/src/main/scala/hu/sztaki/ilab/mf,
 * core = core/src/main/scala/hu/sztaki/ilab/recom/core,
 * sp = spark-adaptive-recom/src/main/scala/hu/sztaki/ilab/recom/spark).
 *
 * Conventions
 *  - Every call returns an int status: MF_OK (0) or a negative MF_ERR_*.
 *    mf_last_error() returns a thread-local message for the last failing call.
 *    The JNI shim maps a non-zero status to RuntimeException, like the reference
 *    (fl/mf/offline/MatrixFactorization.scala:189-190, 270-271).
 *  - Host buffers are caller-owned and never retained past the call.  Device state
 *    (factor slabs, rating blocks, schedules) is owned by the mf_ctx.
 *  - One mf_ctx is not thread-safe; distinct contexts are.
 *  - Ids are the reference's Int ids (user / item id spaces are separate).
 *  - Factor vectors cross the boundary as row-major double[count * k] (the JVM's
 *    Array[Double]); FAST_F32 mode stores f32 on the device and widens on the way out.
 */
#ifndef MFHIP_H
#define MFHIP_H

#include <stdint.h>

/* Testing hooks (schedule and ring invariants, plan digests) are declared in mfhip_testing.h:
   exported by the same library for the test suite, not part of the product surface. */

#ifdef __cplusplus
extern "C" {
#endif

#define MF_OK 0
#define MF_ERR_INVALID (-1)      /* bad argument (IllegalArgumentException)          */
#define MF_ERR_HIP (-2)          /* HIP runtime error                                */
#define MF_ERR_NOT_FITTED (-3)   /* predict before fit (MatrixFactorization.scala:270) */
#define MF_ERR_NO_DEVICE (-4)    /* no usable GPU: the library never falls back to CPU */
#define MF_ERR_COMM (-5)         /* RCCL error                                       */
#define MF_ERR_CAPACITY (-6)     /* caller buffer too small                          */
#define MF_ERR_STATE (-7)        /* call out of order                                */
#define MF_ERR_TIMEOUT (-8)      /* a device-side bound tripped                      */

/* Update arithmetic / precision. */
#define MF_MODE_DETERMINISTIC_F64 0 /* bitwise replay of the reference's update order  */
#define MF_MODE_FAST_F32 1          /* conflict-free rotation schedule, f32 factors    */

/* flink-ml 1.3 LearningRateMethod (fl/mf/offline/DSGDforMF.scala:10,167-169). */
#define MF_LR_DEFAULT 0    /* lr / sqrt(t)                              */
#define MF_LR_CONSTANT 1   /* lr                                        */
#define MF_LR_BOTTOU 2     /* 1 / (lambda * (lr_arg + t - 1))           */
#define MF_LR_INVSCALING 3 /* lr / t^lr_arg                             */
#define MF_LR_XU 4         /* lr * (1 + lambda*lr*t)^-lr_arg            */

/* Factor sides. */
#define MF_SIDE_USER 0
#define MF_SIDE_ITEM 1

/* Online update flavours (core/FactorUpdater.scala; sp/OfflineSpark.scala). */
#define MF_ONLINE_NEXT_FACTORS 0 /* SGDUpdater.nextFactors, ratings in arrival order    */
#define MF_ONLINE_DELTA 1        /* SGDUpdater.delta + "vec + delta" (PS path)          */
#define MF_ONLINE_SPARK_SWEEP 2  /* OfflineSpark.offlineDSGDUpdatesOnly order           */

/* Fast-mode factor blocking (DSGDforMF.scala:531-533 is the reference's). */
#define MF_BLOCKING_REFERENCE 0  /* new Random(id ^ seed).nextInt(numBlocks) (default)   */
#define MF_BLOCKING_BALANCED 1   /* rating-count balanced blocks (faster; different RMSE) */

/* Initialisers for ids first seen online (core/FactorInitializer.scala). */
#define MF_INIT_PSEUDO_RANDOM 0  /* new Random(id), k x nextDouble   (:23-27)           */
#define MF_INIT_SEEDED 1         /* new Random(id ^ seed), as DSGD init (DSGDforMF.scala:548) */

/* ALS regularisation (mf_als_run). */
#define MF_ALS_REG_WEIGHTED 0 /* lambda * n_row on the diagonal: MLlib's ALS-WR, what ALS.train does */
#define MF_ALS_REG_PLAIN 1    /* lambda on the diagonal                                            */

#define MF_UID_BYTES 128         /* RCCL unique id */

/* Parameters mirror MatrixFactorization.scala:201-223 and DSGDforMF.scala:163-169;
   mf_params_init fills the reference defaults. */
typedef struct mf_params {
  int32_t num_factors;     /* NumFactors, default 10                                  */
  int32_t iterations;      /* Iterations, default 10                                  */
  double lambda;           /* Lambda, default 1.0                                     */
  double learning_rate;    /* LearningRate, default 0.001                             */
  int32_t lr_method;       /* MF_LR_*, default MF_LR_DEFAULT                          */
  double lr_arg;           /* Bottou optimalInit / InvScaling,Xu decay                */
  int32_t num_blocks;      /* Blocks, default None -> 1                               */
  int64_t seed;            /* Seed, default Some(0)                                   */
  int32_t has_seed;        /* 1 = Some(seed) (deterministic), 0 = None                */
  int32_t mode;            /* MF_MODE_*, default MF_MODE_DETERMINISTIC_F64            */
  /* online path (core/FactorUpdater.scala:35-54, FactorInitializer.scala) */
  double online_learning_rate; /* SGDUpdater(learningRate), default 0.01               */
  int32_t online_init;         /* MF_INIT_*, default MF_INIT_PSEUDO_RANDOM              */
  /* fast-mode tuning: waves per device for the rotation schedule (0 = auto);
     a negative value -G fixes G rotation groups per rating block */
  int32_t fast_waves;
  /* fast-mode blocking: MF_BLOCKING_REFERENCE (default) or MF_BLOCKING_BALANCED;
     the deterministic mode always uses the reference's blocking */
  int32_t fast_blocking;
  int32_t reserved[6];
} mf_params;

/* Aggregated device statistics (timed with HIP events on the library's stream). */
typedef struct mf_stats {
  int64_t updates;           /* rating updates executed                          */
  int64_t supersteps;        /* DSGD supersteps executed                         */
  int64_t kernel_launches;   /* launches of the dominant (sweep) kernel          */
  double kernel_ms;          /* summed device time of those launches (profiling on) */
  double algorithmic_bytes;  /* updates x B(k) (16k+20 f32, 32k+24 f64)          */
  int64_t levels;            /* deterministic mode: dependency levels launched   */
  int32_t groups;            /* fast mode: rotation groups per rating block      */
  int32_t reserved0;
  int64_t pads;              /* fast mode: no-op records the plan inserted       */
  double moved_bytes;        /* bytes the sweep kernels request from memory: every row load and
                                store they issue (forwarded rows and no-op halves excluded) plus
                                the schedule records they read; an upper bound on HBM traffic */
} mf_stats;

typedef struct mf_ctx mf_ctx;

void mf_params_init(mf_params* p);
const char* mf_last_error(void);
const char* mf_version(void);
int mf_device_count(int* n);

/* Context on n_devices GPUs of this process (device_ids may be NULL -> 0..n-1). */
int mf_create(const mf_params* p, const int* device_ids, int n_devices, mf_ctx** out);
/* Context for one rank of a multi-process job (one process per GPU, RCCL over xGMI).
   uid comes from mf_comm_unique_id on rank 0, shipped to all ranks by the caller. */
int mf_comm_unique_id(uint8_t uid_out[MF_UID_BYTES]);
int mf_create_rank(const mf_params* p, int device_id, int nranks, int rank,
                   const uint8_t uid[MF_UID_BYTES], mf_ctx** out);
int mf_destroy(mf_ctx* ctx);

/* DSGDforMF.fitSGD.fit (fl/mf/offline/DSGDforMF.scala:262-357): blocking, all
   iterations*numBlocks supersteps and unblocking.  Copies the caller's arrays. */
int mf_dsgd_fit(mf_ctx* ctx, const int32_t* users, const int32_t* items, const double* ratings,
                int64_t n);
/* The same fit in stages: prepare (blocking + H2D, :279-337), run supersteps
   (the BulkIteration :341-344; continues the superstep counter across calls),
   and wait for completion.  Resume = mf_set_factors + mf_dsgd_set_superstep. */
int mf_dsgd_prepare(mf_ctx* ctx, const int32_t* users, const int32_t* items, const double* ratings,
                    int64_t n);
int mf_dsgd_run(mf_ctx* ctx, int64_t supersteps);
int mf_dsgd_superstep(mf_ctx* ctx, int64_t* done);
int mf_dsgd_set_superstep(mf_ctx* ctx, int64_t done);
/* Start the prepared fit over: factors back to their initial values (k x nextDouble of
   new Random(id ^ seed), DSGDforMF.scala:548-549) and the superstep counter to 0; blocking
   and the device schedule are kept.  mf_dsgd_run(iterations * numBlocks) then repeats fitSGD. */
int mf_dsgd_restart(mf_ctx* ctx);
int mf_sync(mf_ctx* ctx);

/* unblock (DSGDforMF.scala:245-255) -> factorsOption (MatrixFactorization.scala:64).
   Rows come back in ascending id order. In rank mode only the rows this rank owns. */
int mf_num_factors(mf_ctx* ctx, int side, int64_t* count);
int mf_get_factors(mf_ctx* ctx, int side, int32_t* ids_out, double* vecs_out, int64_t cap,
                   int64_t* written);
/* Overwrite (or, in online use, insert) factor rows (checkpoint restore). */
int mf_set_factors(mf_ctx* ctx, int side, const int32_t* ids, const double* vecs, int64_t n);
/* The context's parameters (e.g. the rank k a caller sizes factor buffers with). */
int mf_get_params(mf_ctx* ctx, mf_params* out);

/* Input and snapshots.
   mf_read_ratings: env.readCsvFile[(Int, Int, Double)](path) (DSGDforMF.scala:72) and MovieLens
   u.data: one "user<d>item<d>rating[<d>...]" record per line, d = delim (',' is Flink's default,
   '\t' u.data, 0 = any run of spaces / tabs / commas), the first skip_lines lines skipped, blank
   lines ignored, extra fields ignored.  users == NULL: only *n_out = record count.  A line
   that does not parse fails with MF_ERR_INVALID naming the line.
   mf_save_model / mf_load_model: the TemporaryPath persistence of the fit (DSGDforMF.scala:291-296,
   330-349) as one binary file: both factor sides (ids ascending, f64) and the superstep counter.
   Loading sets the factors (mf_set_factors semantics) and returns the stored counter; to resume
   a fit: mf_dsgd_prepare (same ratings), mf_load_model, mf_dsgd_set_superstep(counter),
   mf_dsgd_run. */
int mf_read_ratings(const char* path, char delim, int32_t skip_lines, int32_t* users, int32_t* items,
                    double* ratings, int64_t cap, int64_t* n_out);
int mf_save_model(mf_ctx* ctx, const char* path);
int mf_load_model(mf_ctx* ctx, const char* path, int64_t* superstep_out);

/* predictRating (MatrixFactorization.scala:239-274): inner-join semantics via found[]. */
int mf_predict(mf_ctx* ctx, const int32_t* users, const int32_t* items, int64_t n, double* out,
               uint8_t* found);
/* RMSE = sqrt(mean((r - p.q)^2)) over the inner-joined pairs (the reference has none). */
int mf_rmse(mf_ctx* ctx, const int32_t* users, const int32_t* items, const double* ratings,
            int64_t n, double* rmse, int64_t* matched);
/* empiricalRisk (MatrixFactorization.scala:133-192), duplicate-pair join semantics kept. */
int mf_empirical_risk(mf_ctx* ctx, const int32_t* users, const int32_t* items,
                      const double* ratings, int64_t n, double lambda, double* risk);

/* MatrixFactorizationModel.recommendProducts / recommendUsers / recommendProductsForUsers (the
   model sp/OnlineSpark.scala:12, 126 builds): scored and selected on the device.
   query_side = MF_SIDE_USER: for each queries[j] (a user id) the top_n item ids by p.q.
   query_side = MF_SIDE_ITEM: for each item id the top_n user ids.
   ids_out / scores_out (may be NULL): n_queries x top_n, row-major; counts_out[j] = valid entries
   of row j = min(top_n, candidates left after exclusion), 0 for an unknown query id.  Ids may be
   negative, so counts_out is the only validity signal; slots past it hold id 0 and score 0.0.
   (excl_query[e], excl_cand[e]) pairs are never returned for that query; pairs naming an unknown id
   or a query not in queries[] are ignored, duplicates allowed, n_excl == 0 takes NULL pointers.
   A row is sorted by score descending, ties by candidate id ascending, NaN below every number
   (-inf included).  Scores: MF_MODE_DETERMINISTIC_F64 bitwise mf_predict's value of the pair;
   MF_MODE_FAST_F32 the f32 fmaf chain over f = 0..k-1 from 0, widened.
   Single-process contexts only (a rank-mode context returns MF_ERR_STATE). */
#define MF_RECOMMEND_MAX_TOP 128
int mf_recommend(mf_ctx* ctx, int query_side, const int32_t* queries, int64_t n_queries,
                 int32_t top_n,
                 const int32_t* excl_query, const int32_t* excl_cand, int64_t n_excl,
                 int32_t* ids_out, double* scores_out, int32_t* counts_out);

/* Nearest neighbours in factor space, scored and selected on the device like mf_recommend and never
   forming a score matrix.
   mf_similar: "items like this item" / "users like this user".  For each queries[j] (an id of `side`) the
   top_n ids of the SAME side.  Candidates are every row of `side`; with include_self == 0 the query's own
   row is left out, so counts_out[j] = min(top_n, rows - 1 - distinct known exclusions of the query) and a
   side with one row gives count 0; with include_self == 1 the query is a candidate like any other (naming
   the (query, query) pair in the exclusions removes it again, and naming it with include_self == 0 changes
   nothing).  An unknown query id gives count 0; duplicate query ids each take their row's result.
   mf_recommend_vectors: top_n rows of cand_side for query vectors the model does not hold (an anonymous
   session, a row folded in elsewhere, an average of item vectors).  vecs: n_queries x k, row-major,
   k = num_factors, converted to the context's precision exactly as mf_set_factors converts rows (f64 kept,
   f32 by one rounding).  NaN and infinite entries are allowed and follow the ordering rules below.
   excl_query_index[e] names position j of vecs; indices outside [0, n_queries) are ignored.
   Shared with mf_recommend: the output layout (ids_out / scores_out (may be NULL): n_queries x top_n,
   row-major), counts_out as the only validity signal with slots past it holding id 0 and score 0.0; the
   order (score descending, ties by candidate id ascending (signed), NaN below every number, -0 as +0); the
   exclusion rules (pairs naming an unknown id or a query not asked are ignored, duplicates allowed,
   n_excl == 0 takes NULL pointers); top_n in 1 .. MF_RECOMMEND_MAX_TOP; n_queries == 0 is valid; a context
   on several devices uses its first.
   Scores, metric = MF_METRIC_DOT: the value mf_recommend would report if the query row sat on the
   opposite side, the same arithmetic bit for bit -- MF_MODE_DETERMINISTIC_F64 the chain pq = pq + a*b over
   f = 0..k-1, MF_MODE_FAST_F32 the f32 fmaf chain over f = 0..k-1 from 0, widened.
   Scores, metric = MF_METRIC_COSINE, for rows x in the context's precision T (f32 or f64):
     nn(x)  = the sum over ascending f from 0 of x_f * x_f in T: f32 the chain nn = fmaf(x_f, x_f, nn), f64
              nn = nn + x_f * x_f (product rounded, then the sum: not fused)
     inv(x) = 1.0 / sqrt((double)nn), square root and division in f64; f32 then rounds it once to f32
     score  = dot * (inv(query) * inv(candidate)) in T: the product of the two inverses first, each multiply
              rounded once, the result widened to f64; dot is the MF_METRIC_DOT value above (in T)
   This is symmetric bit for bit: score(a, b) == score(b, a).  A zero row has inv = +inf and dot = 0, so its
   score is NaN and it sorts last; whatever IEEE arithmetic gives on overflow or underflow is the answer,
   there is no special casing.  Results are reproducible bit for bit and depend neither on how the queries
   are batched nor on how the candidates are split.  Norms are computed per call and never kept: a row
   changed by mf_set_factors, an online batch or a fit is reflected by the next call.
   Errors.  MF_ERR_INVALID: NULL ctx, a bad side, an unknown metric, an include_self other than 0 or 1,
   top_n outside 1 .. MF_RECOMMEND_MAX_TOP, a negative count, a NULL array with a positive count.
   MF_ERR_NOT_FITTED before a model exists; MF_ERR_STATE on a rank-mode context, as mf_recommend. */
#define MF_METRIC_DOT    0
#define MF_METRIC_COSINE 1
int mf_similar(mf_ctx* ctx, int side, const int32_t* queries, int64_t n_queries, int32_t top_n,
               int32_t metric, int32_t include_self,
               const int32_t* excl_query, const int32_t* excl_cand, int64_t n_excl,
               int32_t* ids_out, double* scores_out /* may be NULL */, int32_t* counts_out);
int mf_recommend_vectors(mf_ctx* ctx, int cand_side, const double* vecs, int64_t n_queries, int32_t top_n,
                         int32_t metric,
                         const int64_t* excl_query_index, const int32_t* excl_cand, int64_t n_excl,
                         int32_t* ids_out, double* scores_out /* may be NULL */, int32_t* counts_out);

/* The top_n WITHIN caller-given candidate lists: "the best 10 among the items in stock", or the second
   stage "rank these 500 retrieved candidates for this user".  mf_recommend restricted, never the complement
   spelled out as exclusion pairs.
   Definition.  Position j of the outputs holds, bit for bit, what
     mf_recommend(ctx, query_side, &queries[j], 1, top_n, E_j, ...)
   returns, where E_j is this call's exclusions plus every pair (queries[j], c) of a candidate row c the model
   holds whose id is NOT in list j.  Ids, scores, counts, the order (score descending, ties by candidate id
   ascending (signed), NaN below every number, -0 as +0) and the output layout (ids_out / scores_out (may be
   NULL): n_queries x top_n, row-major; counts_out the only validity signal, slots past it id 0 and score 0.0)
   are mf_recommend's.
   Lists.  offsets == NULL: every query uses cand_ids[0 .. n_cand) -- the allow-list.  Otherwise query j owns
   cand_ids[offsets[j] .. offsets[j + 1]): offsets holds n_queries + 1 entries, offsets[0] == 0, never
   decreasing, offsets[n_queries] == n_cand.  An id the candidate side does not hold is dropped; an id named
   several times counts once; an empty list gives count 0; an unknown query id gives count 0; duplicate query
   ids each take their own position's list.  So
     counts_out[j] = min(top_n, distinct held ids of list j - those of them excluded for queries[j]).
   Exclusions.  exclude_seen == 0: the excl_* arrays under mf_recommend's rules (pairs naming an unknown id or
   a query not asked are ignored, duplicates allowed, n_excl == 0 takes NULL pointers; a pair may name a
   candidate outside the list).  exclude_seen == 1: the resident seen set of query_side exactly as
   mf_recommend_seen reads it -- no set, or an empty one, means no exclusions -- and n_excl must be 0.
   Scores.  mf_recommend's arithmetic: MF_MODE_DETERMINISTIC_F64 the chain pq = pq + a*b over f = 0..k-1 (not
   fused), MF_MODE_FAST_F32 the f32 fmaf chain over f = 0..k-1 from 0, widened.  Results depend neither on how
   the queries are batched nor on how the lists are cut into parts, and a shared list gives what the same list
   repeated for every query gives.  Nothing in the context changes.
   Errors, all raised before the context is read.  MF_ERR_INVALID: a NULL ctx, a bad side, top_n outside
   1 .. MF_RECOMMEND_MAX_TOP, a negative count, n_queries or n_cand >= 2^31, a NULL array with a positive count
   (offsets may be NULL: that is the shared list), offsets[0] != 0, decreasing offsets, offsets[n_queries] !=
   n_cand, an exclude_seen other than 0 or 1, exclude_seen == 1 with n_excl > 0.  Then MF_ERR_NOT_FITTED before
   a model exists and MF_ERR_STATE on a rank-mode context, as mf_recommend.  n_queries == 0 is valid; a context
   on several devices uses its first. */
int mf_recommend_among(mf_ctx* ctx, int query_side, const int32_t* queries, int64_t n_queries, int32_t top_n,
                       const int64_t* offsets /* [n_queries + 1], or NULL: one shared list */,
                       const int32_t* cand_ids, int64_t n_cand,
                       int32_t exclude_seen,
                       const int32_t* excl_query, const int32_t* excl_cand, int64_t n_excl,
                       int32_t* ids_out, double* scores_out /* may be NULL */, int32_t* counts_out);

/* RankingMetrics (precisionAt, meanAveragePrecision, ndcgAt) of MLlib, for the models ALS.train builds
   (sp/OnlineSpark.scala:125-131), plus recall, reciprocal rank and hit rate: held-out (query,
   candidate) pairs against the model's top-N lists, on the device.  The pair tables are built, the
   lists scored and selected, the per-query metrics taken and summed there; only the metrics cross to
   the host.
   Evaluated queries.  The distinct ids of gt_query[] the model holds on query_side.  Each has its
   ground-truth set G = the distinct gt_cand ids paired with it, g = |G| >= 1.  A ground-truth
   candidate the model does not hold still counts in G (it can never be hit); duplicate pairs count
   once.  Distinct unknown query ids are counted in unknown_queries and take no part in the means.
   Lists.  The list L of a query is exactly what mf_recommend(ctx, query_side, that id, top_n,
   excl_query, excl_cand, n_excl, ...) returns: the same scores, the same order (score descending,
   ties by id ascending, NaN last), the same exclusion rules, count c <= N = top_n.  A pair that is
   both excluded and in G stays in G and is never hit.
   Per query, with h_i = [L_i in G] for i = 0 .. c-1, in f64, every sum taken sequentially over
   ascending i:
     hits      = sum h_i
     precision = hits / N            (N even when c < N, as MLlib's precisionAt)
     recall    = hits / g
     ap        = (sum over hit positions i of cnt_i / (i + 1)) / g, cnt_i = hits up to and including i
                 (MLlib 2.2's meanAveragePrecision applied to the N-list)
     ndcg      = dcg / idcg, gain_i = 1 / log(i + 2) (natural log), dcg = sum_{h_i} gain_i,
                 idcg = sum_{i < min(g, N)} gain_i  (MLlib's ndcgAt reduces to this)
     rr        = 1 / (position of the first hit + 1), 0 with no hit
     hit       = 1.0 if hits > 0 else 0.0
   The 128 gains and their 129 prefix sums are computed once on the host with libm's log and uploaded;
   no device log is called, so a host replay with the same libm matches bit for bit.
   Aggregates.  Each mean is (sum over the evaluated queries) / queries; queries == 0 gives all zeros,
   not NaN.  The sums are taken in a fixed order: the per-query values in ascending factor-row order of
   the queries, in slices of 1024 with a fixed pairwise tree inside a slice, the slices added in
   ascending order; no floating-point atomics.  Results are bitwise reproducible from run to run and do
   not depend on how the queries are batched or the candidates split.
   Per-query outputs (optional: all three pointers NULL, or all given, with room for cap rows): rows in
   ascending query id; q_ids_out[cap], q_counts_out[cap][2] = (hits, g),
   q_metrics_out[cap][MF_RANK_NMETRICS] = precision, recall, ap, ndcg, rr, hit.  cap < queries returns
   MF_ERR_CAPACITY with the needed count in out->queries and in the message.
   Errors.  MF_ERR_INVALID: NULL ctx or out, a bad side, top_n outside 1 .. MF_RECOMMEND_MAX_TOP, a
   negative count, a NULL array with a positive count, some but not all per-query pointers.
   MF_ERR_NOT_FITTED before a model exists; MF_ERR_STATE on a rank-mode context, as mf_recommend.
   n_gt == 0 is valid and gives all zeros.  A context on several devices evaluates on its first. */
typedef struct mf_rank_metrics {
  int64_t queries;          /* evaluated queries */
  int64_t unknown_queries;  /* distinct ground-truth query ids the model does not hold */
  int64_t gt_pairs;         /* distinct ground-truth pairs of the evaluated queries */
  int64_t hits;             /* ground-truth candidates found in the top-N lists */
  double precision, recall, map, ndcg, mrr, hit_rate;   /* means over `queries` */
  double reserved[6];
} mf_rank_metrics;
#define MF_RANK_NMETRICS 6   /* precision, recall, ap, ndcg, rr, hit -- per-query row layout */
int mf_rank_eval(mf_ctx* ctx, int query_side,
                 const int32_t* gt_query, const int32_t* gt_cand, int64_t n_gt,
                 int32_t top_n,
                 const int32_t* excl_query, const int32_t* excl_cand, int64_t n_excl,
                 mf_rank_metrics* out,
                 int32_t* q_ids_out, int32_t* q_counts_out, double* q_metrics_out, int64_t cap);

/* The position of given (query, candidate) pairs in the query's complete ranked list, computed on the
   device without building the list (a fused score-and-count): what prequential evaluation, the expected
   percentile rank of the implicit-feedback literature and a check of mf_recommend past its first 128
   positions need.
   For pair j, rank_out[j] is the 0-based position cands[j] takes in the complete list of queries[j]:
   every candidate row the model holds on the other side, minus the exclusions of that query, ordered
   exactly as mf_recommend orders (score descending, ties by candidate id ascending (signed), NaN below
   every number, -0 tied with +0).  Put differently: the number of non-excluded candidates other than
   cands[j] whose key beats the pair's key.  score_out[j] (may be NULL) is the score mf_recommend reports
   for the pair: MF_MODE_DETERMINISTIC_F64 mf_predict's value, MF_MODE_FAST_F32 the f32 fmaf chain over
   f = 0..k-1 from 0, widened (in both, as there, a NaN is the canonical quiet NaN and -0 reads +0).  So for
   every N <= MF_RECOMMEND_MAX_TOP, rank_out[j] < N holds exactly when cands[j] is entry rank_out[j] of
   mf_recommend(queries[j], N, the same exclusions), and score_out[j] is that entry's score bit for bit.
   valid_out[j] (may be NULL) is the length of that complete list: the candidate rows minus the distinct
   excluded candidates of the query that the model holds; >= 1 for a ranked pair.
   A pair whose query id or candidate id the model does not hold gets MF_PAIR_RANK_COLD, a pair that is
   itself in the exclusion list MF_PAIR_RANK_EXCLUDED; both with valid_out 0 and score_out 0.0.
   Exclusion pairs follow mf_recommend's rules: unknown ids ignored, duplicates allowed, pairs naming a
   query not in queries[] ignored.  Every pair is ranked independently: duplicates in queries / cands are
   allowed, output order is input order.  Results do not depend on how the pairs are batched or the
   candidates split and are reproducible bit for bit (counts are integers).
   Errors and state rules are mf_recommend's: MF_ERR_INVALID (NULL ctx, a bad side, a negative count, a
   NULL array with a positive count), MF_ERR_NOT_FITTED, MF_ERR_STATE on a rank-mode context.  A context
   on several devices evaluates on its first.  n == 0 is valid. */
#define MF_PAIR_RANK_COLD     (-1)  /* the model does not hold the query id or the candidate id */
#define MF_PAIR_RANK_EXCLUDED (-2)  /* the pair itself is in the exclusion list */
int mf_pair_ranks(mf_ctx* ctx, int query_side,
                  const int32_t* queries, const int32_t* cands, int64_t n,
                  const int32_t* excl_query, const int32_t* excl_cand, int64_t n_excl,
                  int32_t* rank_out,      /* [n] */
                  int32_t* valid_out,     /* [n] or NULL */
                  double*  score_out);    /* [n] or NULL */

/* Prequential (test-then-train) evaluation of the online path, the "online DCG" online recommenders are
   judged by: every event of a micro-batch is ranked with the model as it stands, then the model learns
   the batch.
   Step 1 ranks all n events with mf_pair_ranks(ctx, MF_SIDE_USER, users, items, n, excl_user, excl_item,
   n_excl, ...) against the model as it stands on entry (micro-batch prequential: no event of the batch
   sees another event of the batch; n = 1 gives strict test-then-train).  rank_out (may be NULL) receives
   those ranks and codes.  A context that holds no model yet is not an error: every event is cold.
   Step 2 performs exactly mf_online_update(ctx, users, items, ratings, n, flavour, num_partitions,
   touched_users, touched_items): the model afterwards is bitwise what mf_online_update alone leaves.
   Per evaluated event with rank r and list length V, N = top_n in 1 .. MF_RECOMMEND_MAX_TOP, in f64:
     ndcg = gain[r] / idcg[1] for r < N, else 0: mf_rank_eval's table, so bitwise mf_rank_eval's per-query
            ndcg of a query whose ground truth is this one item (mathematically 1 / log2(r + 2))
     rr   = 1 / (r + 1) for r < N, else 0
     hit  = [r < N]
     pr   = r / (V - 1), 0 when V = 1: the expected percentile rank (Hu, Koren, Volinsky); not cut at N
   Cold and excluded events contribute 0.0.  The three sums are taken over the events in ascending j, in
   slices of 1024 with a fixed pairwise tree inside a slice, the slices added in ascending order
   (mf_rank_eval's order); no floating-point atomics.  The sums are returned beside the means so that a
   caller adds batches exactly.
   Errors: mf_online_update's own; top_n out of range; a NULL out; a NULL array with a positive count;
   MF_ERR_STATE on a rank-mode context.  Validation runs before anything is updated: a failing call
   leaves the model untouched. */
typedef struct mf_prequential {
  int64_t events, evaluated, cold, excluded, hits;   /* events = n = evaluated + cold + excluded */
  double sum_ndcg, sum_rr, sum_pr;                   /* sums over the evaluated events */
  double ndcg, mrr, hit_rate, mpr;                   /* sums / evaluated; 0 when evaluated == 0 */
  double reserved[6];
} mf_prequential;
int mf_online_prequential(mf_ctx* ctx, const int32_t* users, const int32_t* items, const double* ratings,
                          int64_t n, int flavour, int num_partitions, int32_t top_n,
                          const int32_t* excl_user, const int32_t* excl_item, int64_t n_excl,
                          mf_prequential* out, int32_t* rank_out /* [n] or NULL */,
                          int64_t* touched_users, int64_t* touched_items);

/* ALS.train(ratings, rank = params.num_factors, iterations, lambda), the "ALS" branch of
   OnlineSpark.buildModelCombineOffline (sp/OnlineSpark.scala:125-131), as alternating least squares
   on the device.  mf_als_prepare keeps the ratings on the device as one CSR per side (the ratings of
   a row in the order of the caller's arrays); mf_als_run runs half-sweeps; mf_als_fit is
   mf_als_prepare followed by mf_als_run(2 * iterations).  n == 0 makes mf_als_fit a no-op.
   Order and arithmetic.  A half-sweep solves, for every row a of one side with at least one rating,
       (sum_j q_j q_j^T + lambda' I) x = sum_j r_j q_j
   over that row's ratings j (duplicate pairs included), q_j the counterpart's row as it stands when
   the half-sweep begins; lambda' = lambda * n_a (n_a = the row's rating count) for
   MF_ALS_REG_WEIGHTED and lambda' = lambda for MF_ALS_REG_PLAIN.  The solve is a Cholesky
   factorisation and two triangular solves; a pivot that is not a positive finite number makes that
   row NaN.  Half-sweep 0 solves the item side from the user factors, half-sweep 1 the user side from
   the item factors, and so on alternately (MLlib's order); the counter starts at 0 in mf_als_prepare
   and continues across mf_als_run calls.  MF_MODE_DETERMINISTIC_F64 contexts compute in f64,
   MF_MODE_FAST_F32 contexts in f32 throughout (ratings and lambda rounded to f32).  Results are
   bitwise reproducible from run to run.
   Model.  Rows the context already holds are kept (a warm start: the online + offline combination);
   ids not yet in the model are inserted under mf_online_update's rules for a fitted or prepared
   context, with the initial values mf_dsgd_fit gives them (k x nextDouble of new Random(id ^ seed)).
   Rows with no rating in the data are left untouched.  After a run the context is fitted.
   MLlib's own initial factors (normalised |Gaussian| draws from a per-partition XORShift stream)
   are NOT reproduced: MLlib is not part of the reference tree and its stream depends on Spark's
   partitioning, so factors agree with MLlib's in quality, not in bits.
   Errors.  MF_ERR_INVALID: lambda <= 0, a negative count, an unknown reg, or a rank above 256 (up
   to 128 the k x k normal matrix of a row is kept in LDS, from 129 to 256 in global memory).
   MF_ERR_STATE: mf_als_run before mf_als_prepare (or after a later mf_dsgd_prepare / mf_dsgd_fit,
   which rebuilds the rows), a rank-mode context, or a context on more than one device. */
int mf_als_fit(mf_ctx* ctx, const int32_t* users, const int32_t* items, const double* ratings, int64_t n,
               int32_t iterations, double lambda, int32_t reg);
int mf_als_prepare(mf_ctx* ctx, const int32_t* users, const int32_t* items, const double* ratings,
                   int64_t n);
int mf_als_run(mf_ctx* ctx, int64_t half_sweeps, double lambda, int32_t reg);

/* ALS.trainImplicit(ratings, rank, iterations, lambda, alpha): the confidence-weighted factorisation
   of implicit feedback (Hu, Koren, Volinsky 2008) as MLlib runs it.  mf_als_prepare is shared and
   unchanged; mf_als_run_implicit runs half-sweeps on the prepared data, mf_als_fit_implicit is
   mf_als_prepare followed by mf_als_run_implicit(2 * iterations) (n == 0: a no-op).
   Arithmetic.  A half-sweep solves, for every row a of one side with at least one rating,
       (G + sum_j w_j q_j q_j^T + lambda' I) x = sum_{j : r_j > 0} (1 + w_j) q_j,   w_j = alpha * |r_j|
   The sums run over that row's ratings j in CSR order, duplicate pairs included; q_j is the
   counterpart's row as it stands when the half-sweep begins.  G = sum_b y_b y_b^T runs over the
   counterpart rows b with at least one rating in the prepared data (the rows MLlib has factors
   for): rows the context holds but the data does not name take no part in G and are left untouched.
   This is MLlib's rule (c1 = alpha * |r|; ls.add(q, if r > 0 then 1 + c1 else 0, c1)): a rating of 0
   contributes nothing, a negative rating adds confidence to a preference of 0.
   lambda' = lambda * n+_a for MF_ALS_REG_WEIGHTED, n+_a the number of the row's ratings with r > 0
   (MLlib's numExplicits), and lambda' = lambda for MF_ALS_REG_PLAIN.  A row whose ratings are all
   <= 0 has a zero right-hand side: it is set to zero without factorising (the exact solution of a
   nonsingular system, also where lambda' = 0).
   Order.  The rating sum is taken per chunk in CSR order, chunks ascending, exactly as mf_als_run
   takes it; then + G; then + lambda' on the diagonal.  Only the lower triangle is formed, the weight
   multiplying one operand -- (w_j q_j[a]) * q_j[b] with a >= b -- so the matrix is symmetric by
   construction.  G itself is summed over the rated rows in ascending row order, in slices of 1024
   rows whose partial sums are added in ascending order.  Deterministic contexts compute in f64,
   fast contexts in f32 throughout (alpha, lambda and the ratings rounded to f32).  Results are
   bitwise reproducible from run to run.  mf_als_run's rule for a pivot that is not a positive
   finite number holds.  The half-sweep order and the counter are mf_als_run's, and the two kinds
   of run call share the counter: the item side first, 0 after mf_als_prepare, continuing across calls.
   Errors.  MF_ERR_INVALID: alpha < 0 or not finite (alpha = 0 is valid); otherwise exactly
   mf_als_run's / mf_als_fit's. */
int mf_als_run_implicit(mf_ctx* ctx, int64_t half_sweeps, double lambda, int32_t reg, double alpha);
int mf_als_fit_implicit(mf_ctx* ctx, const int32_t* users, const int32_t* items, const double* ratings,
                        int64_t n, int32_t iterations, double lambda, int32_t reg, double alpha);

/* The same half-sweeps by conjugate gradients (Hu, Koren, Volinsky 2008 with the solve of Takacs,
   Pilaszy, Tikk 2011): every rated row takes cg_steps CG steps on its normal equations, starting from
   its current value, and its k x k matrix is never formed.  About 4 (cg_steps + 1) nnz k flops per
   half-sweep instead of 2 nnz k^2 and a factorisation per row; an approximate solve, exact in at most k
   steps in exact arithmetic.  Every rank 1..256 runs the same kernels.
   Shared with mf_als_run / mf_als_run_implicit: the data mf_als_prepare built, the half-sweep order
   (item side first) and the half-sweep counter -- the four kinds of run call may be mixed --, the state
   rules and errors, lambda', n+ and G, and that a row with no rating is left untouched and every row of
   a half-sweep reads the counterpart's factors as they stand when the half-sweep begins.
   mf_als_fit_cg / mf_als_fit_implicit_cg are mf_als_prepare followed by the run call with
   2 * iterations half-sweeps (n == 0: a no-op).
   Arithmetic.  Per row a with ratings j in CSR order, counterpart rows q_j, current value x, S = cg_steps:
       explicit:  A = sum_j q_j q_j^T + lambda' I           b = sum_j r_j q_j
       implicit:  A = G + sum_j w_j q_j q_j^T + lambda' I   b = sum_j c_j q_j
                  w_j = alpha |r_j|,  c_j = 1 + w_j where r_j > 0 and 0 elsewhere
       r = b - A x, in one pass:  r = sum_j e_j q_j [- G x] - lambda' x,  e_j = r_j - q_j.x  (implicit: c_j - w_j (q_j.x))
       p = r;  rs = r.r
       S times:  Ap = sum_j e_j q_j [+ G p] + lambda' p,  e_j = q_j.p  (implicit: w_j (q_j.p))
                 a = rs / (p.Ap);  x = fma(a, p, x);  r = fma(-a, Ap, r);  rs' = r.r;  p = fma(rs'/rs, p, r);  rs = rs'
   An implicit row with no positive rating is set to +0 without iterating.  Before a step, rs == 0 ends the
   row's iterations and keeps x; so does p.Ap == 0.  An rs or p.Ap that is not finite makes the row NaN
   (mf_als_run's rule for a bad pivot).
   Order.  q_j.v: 64 partial sums, partial l an fma chain from 0 over f = l, l + 64, l + 128, l + 192 (< k),
   added pairwise: partial l with l ^ 32, then ^ 16, ^ 8, ^ 4, ^ 2, ^ 1.  sum_j e_j q_j: per factor an fma chain from 0
   over the ratings in CSR order; a row longer than the chunk of mf_als_prepare takes one such chain per
   chunk and adds the chunks' sums to 0 in ascending order.  (G v)[f]: an fma chain from 0 over g = 0 .. k-1
   of G[g][f] v[g].  Then, in this order, [-/+ G v] and -/+ lambda' v (a product, then a sum).  r.r and
   p.Ap: the products of factors 64 g .. 64 g + 63 form group g = 0 .. 3 (factors past k count 0), each
   group is added by the same pairwise scheme, then ((g0 + g1) + g2) + g3.  Deterministic contexts
   compute in f64, fast contexts in f32 throughout (lambda, alpha and the ratings rounded to f32).
   No floating-point atomics: results are bitwise reproducible from run to run and do not depend on the
   device, on how the rows are cut into launches, or on whether a row's vectors were kept on chip; they
   depend on the chunk length as mf_als_run's do.
   Errors.  MF_ERR_INVALID: cg_steps outside 1 .. MF_ALS_CG_MAX_STEPS; otherwise exactly those of
   mf_als_run / mf_als_run_implicit / mf_als_fit / mf_als_fit_implicit. */
#define MF_ALS_CG_MAX_STEPS 256
int mf_als_run_cg(mf_ctx* ctx, int64_t half_sweeps, double lambda, int32_t reg, int32_t cg_steps);
int mf_als_run_implicit_cg(mf_ctx* ctx, int64_t half_sweeps, double lambda, int32_t reg, double alpha,
                           int32_t cg_steps);
int mf_als_fit_cg(mf_ctx* ctx, const int32_t* users, const int32_t* items, const double* ratings, int64_t n,
                  int32_t iterations, double lambda, int32_t reg, int32_t cg_steps);
int mf_als_fit_implicit_cg(mf_ctx* ctx, const int32_t* users, const int32_t* items, const double* ratings,
                           int64_t n, int32_t iterations, double lambda, int32_t reg, double alpha,
                           int32_t cg_steps);

/* Non-negative ALS (MLlib's ALS with nonnegative = true): the same half-sweeps with every row solved for
   x >= 0 by a projected conjugate-gradient non-negative least squares (NNLS) in the family of MLlib's
   NNLS.scala, on the row's k x k matrix where the Cholesky half-sweep keeps it (LDS up to rank 128,
   global memory from 129 to 256).
   Shared with the other six run calls: the data mf_als_prepare built, the half-sweep order (item side
   first) and the half-sweep counter -- all eight kinds of run call may be mixed --, the state rules and
   errors (ranks 1 to 256), the formation of the row's system (mf_als_run's, and with alpha
   mf_als_run_implicit's: the sums, their order, the chunks, G, lambda' and n+), and that a row with no
   rating is left untouched.  mf_als_fit_nonneg / mf_als_fit_implicit_nonneg are mf_als_prepare followed
   by the run call with 2 * iterations half-sweeps (n == 0: a no-op).
   The solve.  For a row with A (k x k, symmetric positive definite, lambda' already on the diagonal, G
   added for implicit rows; the upper triangle is a copy of the lower) and b, in the context's precision
   T, with proj(res, x) = res with entry i zeroed wherever res_i > 0 and x_i == 0:
       x = 0;  bb = b.b;  lastWall = 0;  lastDir = 0;  lastNorm = 0
       cap = max(400, 20 k);   tol2 = 1e-12 (rounded to T);   slack = 1 - 64 eps(T)
       for it = 0 .. cap-1:
           res = A x - b
           g   = proj(res, x);   ng = g.g
           dir = g;  step = (g.res) / (g.(A g));  nd = ng
           if it > lastWall + 1:
               d2 = fma(ng / lastNorm, lastDir, g);  s2 = (d2.res) / (d2.(A d2));  n2 = d2.d2
               if not stop(s2, n2):  dir, step, nd = d2, s2, n2
           if nd <= tol2 * bb: done, reason 0;  else if step is not finite: done, reason 3;
           else if not step > 0: done, reason 2
           for i ascending:  if step * dir_i > x_i:  step = x_i / dir_i            (do not cross a wall)
           for i:  if step * dir_i > x_i * slack:  x_i = +0, lastWall = it
                   else x_i = x_i - step * dir_i
           lastDir = dir;  lastNorm = ng
       stop(step, nd):  step is not finite,  or step <= 0,  or nd <= tol2 * bb
   The stopping rule is relative to b.b, so the solve is scale-free: (A, b) times a power of two gives the
   same x and the same iteration count bit for bit.  (MLlib's absolute thresholds step < 1e-7 and
   |dir|^2 < 1e-12 |x|^2 are not; they never fire in f32.)  Every row ends with a reason code:
       0  converged (nd <= tol2 * bb)            x
       1  hit the iteration cap                  x as it stands
       2  step <= 0                              x as it stands
       3  a non-finite step or bb                the whole row is NaN (mf_als_run's rule for a bad pivot)
   A bb that is not finite ends the row before it = 0 with reason 3.  The iteration count of a row is the
   number of updates of x: `it` when the row is done, cap for reason 1.  A row with b <= 0 everywhere ends
   at it = 0 with x = +0 and reason 0.  An implicit row with no positive rating is set to +0 without
   iterating.  Every entry that leaves the solver is >= 0 and never -0 (x starts at +0, a wall
   stores +0, and x_i - step * dir_i cannot round to -0).
   Order, a function of k alone.  (A v)[i]: an fma chain from 0 over j = 0 .. k-1 of A[j][i] v[j].  Every
   dot product u.v: 64 partial sums, partial l an fma chain from 0 over f = l, l + 64, l + 128, l + 192
   (< k) of u[f] v[f], added pairwise: partial l with l ^ 32, then ^ 16, ^ 8, ^ 4, ^ 2, ^ 1.  res_i =
   (A x)[i] - b_i; d2_i is one fma; step * dir_i is a product and x_i - step * dir_i a difference of it;
   the wall clamp runs over i ascending with the step as the earlier entries left it.  Every other
   operation is a single rounding.  Deterministic contexts compute in f64, fast contexts in f32
   throughout.  No floating-point atomics: results are bitwise reproducible from run to run and do not
   depend on the device or on how the rows are cut into launches; they depend on the chunk length only
   through A and b, as mf_als_run's do.
   Errors.  Exactly those of mf_als_run / mf_als_run_implicit / mf_als_fit / mf_als_fit_implicit. */
int mf_als_run_nonneg(mf_ctx* ctx, int64_t half_sweeps, double lambda, int32_t reg);
int mf_als_run_implicit_nonneg(mf_ctx* ctx, int64_t half_sweeps, double lambda, int32_t reg, double alpha);
int mf_als_fit_nonneg(mf_ctx* ctx, const int32_t* users, const int32_t* items, const double* ratings, int64_t n,
                      int32_t iterations, double lambda, int32_t reg);
int mf_als_fit_implicit_nonneg(mf_ctx* ctx, const int32_t* users, const int32_t* items, const double* ratings,
                               int64_t n, int32_t iterations, double lambda, int32_t reg, double alpha);
/* What the non-negative half-sweeps did since mf_als_prepare, from integer counters on the device:
   rows = rows solved (implicit rows set to zero without a solve included, with 0 iterations),
   iterations = the sum of their iteration counts, max_iterations = the longest solve, capped / reason2 /
   nan_rows = rows that ended with reason 1 / 2 / 3.  MF_ERR_STATE before mf_als_prepare. */
struct mf_als_nonneg_stats {
  int64_t rows, iterations, max_iterations, capped, reason2, nan_rows;
};
int mf_als_nonneg_stats(mf_ctx* ctx, struct mf_als_nonneg_stats* out);
/* The solve above on the host (no GPU needed), in the stated order, in f32 (f64 == 0: A and b are rounded
   to f32 first) or f64 arithmetic: the replay the kernels are checked against bit for bit.  A is k x k,
   row-major; only its lower triangle is read.  x_out[k]; iters_out and reason_out may be NULL.
   MF_ERR_INVALID: k outside 1 .. 256 or a null A, b or x_out. */
int mf_nnls_solve(int32_t k, const double* A /* k*k symmetric */, const double* b, int f64, double* x_out,
                  int32_t* iters_out, int32_t* reason_out);

/* Incremental ALS, the ALS side of "combination of online and offline MF" (sp/OnlineSpark.scala:26-162 with
   offlineAlgorithm = "ALS"): new ratings join the CSRs mf_als_prepare left on the device, and only the rows
   they touch are solved again.  Nothing is uploaded but the batch.
   mf_als_solve names one of the eight kinds of half-sweep: {lambda, reg} as in mf_als_run; implicit != 0 with
   alpha as in mf_als_run_implicit (alpha is read only then); solver = MF_ALS_SOLVER_CHOLESKY, _CG (cg_steps as
   in mf_als_run_cg, read only then) or _NNLS (mf_als_run_nonneg).  Set reserved to 0.

   mf_als_append.  Afterwards the prepared data is exactly what mf_als_prepare would have built from the
   earlier arrays followed by these n ratings: per row, on each side, the old ratings in their old order, then
   the new ones in the order of the caller's arrays, duplicate pairs kept.  Ids the model does not hold get
   rows and initial values under mf_als_prepare's rules in every respect (first-touch order, the user looked
   at before the item within one rating; k x nextDouble of new Random(id ^ seed); the same effect on a
   prepared fast DSGD schedule).  Rows the model gained since the last prepare or append through any other
   call (mf_online_update, mf_set_factors) have no ratings until some are appended.  The per-row count and
   the per-row n+ are those of the whole row; n+ counts the ratings > 0 after rounding to the context's
   precision.  The long-row chunks, the launches and the rated-row list that G is summed over are rebuilt as
   mf_als_prepare builds them, with the chunk, batch, Gram-slice and slab values that prepare read.  The
   half-sweep counter and mf_als_nonneg_stats are not reset.  n == 0 is a valid no-op.
   Both CSRs are repacked on the device into fresh arrays (integer moves only, each old entry read once and
   written once; the batch alone is sorted), so a call needs room for a second copy of the larger CSR.
   Errors, all raised before anything changes.  MF_ERR_STATE: before mf_als_prepare, or after a later
   mf_dsgd_prepare / mf_dsgd_fit (a prepare with n = 0 is the valid empty start).  MF_ERR_INVALID: n < 0,
   n >= 2^31, a NULL array with n > 0, or a row that would pass 2^31 - 1 ratings.  Otherwise mf_als_prepare's.

   mf_als_run_rows solves the rows of `side` named by ids[0 .. n_ids), each exactly as a full half-sweep of
   that side with the same `how` would solve it now: the system, the order of every sum, the chunks, G over
   the counterpart's rated rows, lambda' and n+, the NaN rules and the NNLS reason codes.  Every solved row
   reads the counterpart's factors as they stand on entry; every other row keeps its bits.  Ids the model
   does not hold and ids with no rating in the prepared data are skipped; duplicates are solved once;
   *solved_out (may be NULL) is the number of rows solved.  Results do not depend on the order of ids[].
   The half-sweep counter does not move.  NNLS rows count in mf_als_nonneg_stats as a half-sweep's do.
   Errors.  What the mf_als_run* call of the same `how` raises (lambda <= 0, a bad reg, alpha < 0 or not
   finite when implicit, cg_steps outside 1 .. MF_ALS_CG_MAX_STEPS for MF_ALS_SOLVER_CG, a rank above 256,
   the state errors), and MF_ERR_INVALID for a bad side, an unknown solver, a NULL `how`, n_ids < 0, or NULL
   ids with n_ids > 0.

   mf_als_update is, by definition: every argument checked, then mf_als_append(users, items, ratings, n), then
   `rounds` times { mf_als_run_rows(MF_SIDE_USER, the batch's users), mf_als_run_rows(MF_SIDE_ITEM, the
   batch's items) }.  Users go first -- on purpose not MLlib's item-first order of a full sweep: a new user's
   row is random until it is solved, and items solved from it first would be pulled towards noise.
   rounds == 0 is an append; rounds < 0 is MF_ERR_INVALID.  *solved_users_out / *solved_items_out (may be
   NULL) are the counts of the last round (0 with rounds == 0).  With the ratings of one new user and
   rounds = 1 this is fold-in that keeps the user; mf_als_foldin below is the fold-in that keeps nothing. */
#define MF_ALS_SOLVER_CHOLESKY 0
#define MF_ALS_SOLVER_CG 1
#define MF_ALS_SOLVER_NNLS 2
typedef struct mf_als_solve {
  double lambda;
  int32_t reg; /* MF_ALS_REG_* */
  int32_t implicit;
  double alpha;
  int32_t solver; /* MF_ALS_SOLVER_* */
  int32_t cg_steps;
  int32_t reserved[4];
} mf_als_solve;
int mf_als_append(mf_ctx* ctx, const int32_t* users, const int32_t* items, const double* ratings, int64_t n);
int mf_als_run_rows(mf_ctx* ctx, int side, const int32_t* ids, int64_t n_ids, const mf_als_solve* how,
                    int64_t* solved_out /* may be NULL */);
int mf_als_update(mf_ctx* ctx, const int32_t* users, const int32_t* items, const double* ratings, int64_t n,
                  const mf_als_solve* how, int32_t rounds, int64_t* solved_users_out /* may be NULL */,
                  int64_t* solved_items_out /* may be NULL */);

/* Stateless fold-in: the vector a row of `side` would get if its ratings were a list the caller hands over --
   a new visitor's basket, an anonymous session, a cold-start item's first ratings -- solved on the device and
   given back, while the model takes nothing in.  `side` is the side the queries would belong to: with
   MF_SIDE_USER the lists name items and the vectors are user vectors, with MF_SIDE_ITEM the lists name users
   (a new item).  Query j owns entries offsets[j] .. offsets[j + 1] of cand_ids / ratings; offsets has
   n_queries + 1 entries, starts at 0 and never decreases.  Only the lists are uploaded; the ids are resolved,
   the kept entries compacted and (mf_recommend_foldin) the exclusions built on the device.
   Kept entries.  An entry naming an id the counterpart side does not hold is dropped and counts in neither
   the row's count n_a nor its n+; no row is ever inserted.  used_out[j] (may be NULL) is the kept count.
   Duplicates are kept, as mf_als_prepare keeps them.
   The vector.  vecs_out (n_queries x k, row-major, f64; f32 results widened) row j is bit for bit the row
   mf_als_run_rows(side, ..., how) would produce for a row of `side` whose ratings in the prepared data were
   exactly the kept entries in list order: the same system, the same order of every sum, the same long-row
   chunks, the same rules for lambda' (n_a is the kept count), for n+ (counted after rounding to the
   context's precision), for NaN rows and for the NNLS reason codes.  Conjugate gradients start from x = +0.
   A query with no kept entry gives the +0 vector and used_out 0.  Results depend neither on the order of the
   queries nor on how the call batches them.
   G (implicit).  With ALS data prepared, G is summed over the counterpart's rated-row list as it stands (a
   prepare with n = 0 is "prepared": its list is empty and G = 0).  With no ALS data prepared -- a serving
   replica after mf_load_model or mf_set_factors -- G is summed over every counterpart row the model holds, in
   ascending row order and in the same slices, and the long-row chunk length is the one mf_als_prepare would
   read now.
   Nothing changes: factor rows and row numbering, both CSRs and the work lists, the half-sweep counter,
   mf_als_nonneg_stats (the fold-in launches count into scratch counters of their own), the seen set and a
   prepared DSGD schedule are untouched.  A context on one device, single-process.
   mf_recommend_foldin returns what mf_recommend_vectors(cand_side = the other side, the fold-in vectors,
   MF_METRIC_DOT, ...) returns, bit for bit -- ids, scores, counts, order and tie rules, the output layout --
   without the vectors leaving the device (unless vecs_out is given).  exclude_rated != 0: each query's
   distinct kept candidates are its exclusions; 0: there are none.  A query with no kept entry gets count 0,
   and its slots hold id 0 and score 0.0.
   Errors, all raised before any device work.  MF_ERR_INVALID: NULL ctx or `how`; NULL offsets; NULL vecs_out
   (mf_als_foldin), ids_out or counts_out (mf_recommend_foldin) with n_queries > 0; a bad side; n_queries < 0;
   offsets[0] != 0, decreasing offsets, or 2^31 entries or more in total; NULL cand_ids or ratings with
   entries; exclude_rated other than 0 or 1; top_n outside 1 .. MF_RECOMMEND_MAX_TOP; and whatever the
   mf_als_run* call of the same `how` refuses (lambda, reg, alpha, cg_steps, an unknown solver, a rank above
   256).  MF_ERR_NOT_FITTED before a model exists; MF_ERR_STATE on a rank-mode context or one on several
   devices.  n_queries == 0 is valid. */
int mf_als_foldin(mf_ctx* ctx, int side, const int64_t* offsets /* [n_queries + 1] */, const int32_t* cand_ids,
                  const double* ratings, int64_t n_queries, const mf_als_solve* how,
                  double* vecs_out /* n_queries x k */, int32_t* used_out /* [n_queries] or NULL */);
int mf_recommend_foldin(mf_ctx* ctx, int side, const int64_t* offsets, const int32_t* cand_ids,
                        const double* ratings, int64_t n_queries, const mf_als_solve* how, int32_t top_n,
                        int32_t exclude_rated, int32_t* ids_out, double* scores_out /* may be NULL */,
                        int32_t* counts_out, double* vecs_out /* may be NULL */, int32_t* used_out /* may be NULL */);

/* Removal, the mirror image of mf_als_append: ratings leave the CSRs on the device, so that a sliding window,
   a retraction (an un-rated item, a returned purchase, a deleted account, a withdrawn item) needs no
   mf_als_prepare of the surviving history.  The reference's ratingsHistory (sp/OnlineSpark.scala:47,70) is an
   unbounded union; that limitation is not reproduced.  Nothing is uploaded but the batch.

   mf_als_remove.  The rule: the entries are processed in ascending j, and entry j removes the OLDEST remaining
   rating of the pair (users[j], items[j]) -- the first one in the row's CSR order.  CSR order is arrival order
   on both sides, so the user-side and the item-side CSR lose the same instance.  found_out[j] (n bytes, may be
   NULL) = 1 if there was such a rating.  An entry is a miss, and a miss changes nothing, when it names an id
   the model does not hold (no row is ever inserted), a pair that was never rated, or a pair whose instances
   are all gone already; m entries naming one pair remove its m oldest instances.  *removed_out (may be NULL)
   is the number of hits.  The rating values play no part in the choice.
   Resulting state.  The prepared data is exactly what mf_als_prepare would have built from the earlier arrays
   with the removed instances deleted: per row and per side the surviving ratings keep their order; the per-row
   count and n+ are those of what survives (n+ counts the stored values > 0, a comparison on the stored bits
   and the only floating-point operation of the call); the long-row chunks, the launches and the rated-row
   list that G is summed over are rebuilt as mf_als_prepare builds them, with the chunk, batch, Gram-slice and
   slab values that prepare read.  Sliding window: after prepare(A), append(B), append(C), a remove of A's
   (user, item) arrays leaves exactly prepare(B ++ C) on the same rows, even where A and B rate the same pair.
   Emptied rows.  A row that loses its last rating stays in the model and keeps its factor bits; every later
   half-sweep and mf_als_run_rows skip it, and it leaves the rated-row list, so implicit G no longer sums it:
   the rule for rows the data does not name.
   Untouched: factor rows, row numbering, the half-sweep counter, mf_als_nonneg_stats, a prepared fast DSGD
   schedule and the seen set (below: mf_seen_remove, mf_seen_from_als).  The conjugate-gradient work lists are
   rebuilt on their next use, as after an append.
   Each CSR is repacked on the device into fresh arrays, one side at a time (integer work only: the batch is
   sorted, every stored entry searches it, the few that match are ranked by age; every survivor is read once
   and written once), so a call needs room for a second copy of the larger CSR.
   Errors, all raised before anything changes.  MF_ERR_STATE as mf_als_append: before mf_als_prepare, after a
   later mf_dsgd_prepare / mf_dsgd_fit, on a rank-mode context or one with more than one device.
   MF_ERR_INVALID: a NULL ctx, n < 0, n >= 2^31, NULL users / items with n > 0, a rank above 256.  n == 0 is
   a valid no-op with NULL arrays.

   mf_als_remove_rows.  Every rating of the rows of `side` named by ids[0 .. n_ids) leaves both CSRs: an
   account deletion, a withdrawn item.  Ids the model does not hold and ids without ratings are skipped,
   duplicates are allowed; *removed_out (may be NULL) counts the ratings removed, each once.  The resulting
   state and the errors are mf_als_remove's, and MF_ERR_INVALID for a bad side, n_ids < 0 or NULL ids with
   n_ids > 0.  The factor row stays: mf_recommend and every other reader still return it.  Deleting a factor
   row (or renumbering rows) is out of scope.

   mf_als_retract is, by definition: every argument checked as mf_als_update checks them, then
   mf_als_remove(users, items, n, found_out, removed_out), then `rounds` times { mf_als_run_rows(MF_SIDE_USER,
   users), mf_als_run_rows(MF_SIDE_ITEM, items) }.  Users go first for symmetry with mf_als_update (no row is
   new here, so the order carries no hazard).  Rows the removal emptied fall out of mf_als_run_rows by its own
   rule.  rounds == 0 is a remove; rounds < 0 is MF_ERR_INVALID.  *solved_users_out / *solved_items_out (may be
   NULL) are the counts of the last round (0 with rounds == 0). */
int mf_als_remove(mf_ctx* ctx, const int32_t* users, const int32_t* items, int64_t n,
                  uint8_t* found_out /* [n] or NULL */, int64_t* removed_out /* may be NULL */);
int mf_als_remove_rows(mf_ctx* ctx, int side, const int32_t* ids, int64_t n_ids, int64_t* removed_out /* may be NULL */);
int mf_als_retract(mf_ctx* ctx, const int32_t* users, const int32_t* items, int64_t n, const mf_als_solve* how,
                   int32_t rounds, uint8_t* found_out /* [n] or NULL */, int64_t* removed_out /* may be NULL */,
                   int64_t* solved_users_out /* may be NULL */, int64_t* solved_items_out /* may be NULL */);

/* The value of the objective the ALS half-sweeps minimise, on the device, from what mf_als_prepare left there:
   both CSRs, the work lists, the rated-row lists and the factors.  `how` gives lambda, reg, implicit and alpha;
   solver and cg_steps are not read.  The value is that of the prepared data as it stands (after any
   mf_als_append or mf_als_remove) at the factors as they stand.  Nothing is uploaded but the arguments, nothing
   of the context changes (factors, half-sweep counter, seen set, mf_als_nonneg_stats and a prepared DSGD
   schedule keep their state), and the call makes one host synchronisation.  A prepare with n = 0 gives all zeros.

   The arithmetic, defined operation by operation so that it can be replayed bit for bit (mfhip/als.py
   replay_objective).  T is float on a fast context and double on a deterministic one; alpha and lambda are
   rounded to T once.  No operation is fused: every product is rounded before it is added.  Every sum of terms is
   taken in f64.
   dot64(a, b) is step 2 of the mf_bpr_* comment below, unchanged: 64 partials, partial l the chain from 0 over f =
       l, l + 64, ... below k in ascending order, each product rounded before it is added; then v[l] = v[l] +
       v[l ^ 32] for every l at once, then the same with 16, 8, 4, 2, 1; the result is v[0].  (k <= 256.)
   sum64(v[0 .. n)), in f64: lane l chains v[l], v[l + 64], ... from 0.0 in ascending order; then the same
       butterfly; the result is lane 0.
   fit walks the USER side's CSR and work list.  For rating j of user row a (CSR order, duplicates included), with
       q_j the item row: d = dot64(x_a, q_j).  Explicit: e = r - d, t = e * e.  Implicit: w = alpha * |r|; if r >
       0: c = 1 + w, e = 1 - d, t = (c * e) * e - d * d; else t = (w * d) * d -- so a rating of 0 adds exactly 0,
       MLlib's rule as in mf_als_run_implicit.  t is widened to f64.  A work item is a whole row of at most
       als_chunk ratings (mf_als_prepare's chunk length, 16,384) or one chunk of a longer row; it yields sum64 of
       its terms in CSR order.  fit = sum64 of the work items' sums in work-list order (rows ascending, a row's
       chunks ascending).  The chunk length is therefore part of the arithmetic, as it is for mf_bpr_run; the
       launch batch length is not.
   unobserved (implicit only; 0 otherwise).  GU and GI are the two sides' Gram matrices exactly as the implicit
       half-sweeps form them over each side's rated rows.  unobserved = sum64 over e = f * k + g (f, g < k) of
       GU[f][g] * GI[f][g], the product taken in T and then widened.  This is tr(GU GI) = the sum over rated users
       a and rated items b of (x_a . y_b)^2.  A pair rated m times counts once here and m times in fit.
   reg.  Per rated row a of a side, in ascending row order: dot64(x_a, x_a), widened; for MF_ALS_REG_WEIGHTED
       multiplied in f64 by the row's rating count n_a, or when implicit by its count of ratings > 0.  R_side =
       sum64 of these; reg_side = (double)lambda_T * R_side.  Rows with no rating take no part anywhere: the
       half-sweeps never touch them.
   total = ((fit + unobserved) + reg_user) + reg_item.  NaN and infinity propagate; nothing is masked.

   Errors.  MF_ERR_INVALID: NULL ctx, how or out; lambda not finite or below 0 (0 is valid here and gives the
   unregularised loss); an unknown reg; alpha below 0 or not finite when implicit; k above 256.  MF_ERR_STATE: as
   mf_als_run_rows.

   mf_als_run_until is, by definition: every argument checked; J_0 = mf_als_objective(how).total; then for t = 1 ..
   max_iterations: two half-sweeps of the kind `how` names (the run call's own path and counter), J_t = the
   objective, and stop after iteration t if J_t is not finite or J_{t-1} - J_t <= rel_tol * |J_{t-1}|.
   *iterations_out (may be NULL) = the t reached, history_out[0 .. t] (may be NULL) the J values.
   max_iterations == 0 evaluates J_0 and changes nothing.  Errors: mf_als_objective's and the run call's (lambda >
   0 here, cg_steps, an unknown solver), and MF_ERR_INVALID for a negative max_iterations or a rel_tol that is
   negative or not finite; all raised before anything changes. */
typedef struct mf_als_loss {
  double total;       /* ((fit + unobserved) + reg_user) + reg_item */
  double fit;         /* the sum over the prepared ratings */
  double unobserved;  /* implicit: sum over rated users x rated items of (x.y)^2; explicit: 0 */
  double reg_user, reg_item;
  int64_t ratings, user_rows, item_rows;   /* entries summed; rated rows per side */
  double reserved[4];
} mf_als_loss;
int mf_als_objective(mf_ctx* ctx, const mf_als_solve* how, mf_als_loss* out);
int mf_als_run_until(mf_ctx* ctx, const mf_als_solve* how, int32_t max_iterations, double rel_tol,
                     int32_t* iterations_out /* may be NULL */, double* history_out /* [max_iterations + 1] or NULL */);

/* Exact updateLocalFactors replacement (DSGDforMF.scala:378-418) on caller buffers:
   users[nu x k], items[ni x k] are updated in place; omegas are per row.  Reentrant
   on disjoint buffers with distinct contexts, as Flink calls it per task slot. */
int mf_block_update(mf_ctx* ctx, const double* r, const int32_t* uidx, const int32_t* iidx,
                    int64_t len, double* users, const int32_t* uomega, int64_t nu, double* items,
                    const int32_t* iomega, int64_t ni, int k, int iteration, int rating_block_id,
                    int64_t seed, double lr, int lr_method, double lr_arg, double lambda);

/* Online micro-batch (FlinkOnlineMF.scala:112-137 via FactorUpdater.nextFactors;
   PSOfflineOnlineMF.scala:167-180 for MF_ONLINE_DELTA; OnlineSpark.scala:184-229 /
   OfflineSpark.scala:115-207 for MF_ONLINE_SPARK_SWEEP with num_partitions).
   Unseen ids are initialised with params.online_init.  Works on a fitted model too
   (combined offline + online).  Results equal sequential application in the
   flavour's order; touched counts are returned when the pointers are non-NULL. */
int mf_online_update(mf_ctx* ctx, const int32_t* users, const int32_t* items,
                     const double* ratings, int64_t n, int flavour, int num_partitions,
                     int64_t* touched_users, int64_t* touched_items);
/* mf_online_update plus the per-rating records the reference's operators emit, row j of the
   caller's n x k buffers (either may be NULL) for rating j in arrival order:
     MF_ONLINE_NEXT_FACTORS: user_out = nextUserVector, item_out = nextItemVector, the pair
       ItemOperator collects (fl/mf/online/FlinkOnlineMF.scala:131-135);
     MF_ONLINE_DELTA: user_out = userVec + deltaItemVec, the worker's ps.output
       (fl/mf/PSOfflineOnlineMF.scala:176, userVec before this rating's update), item_out =
       deltaItemVec, the vector pushed to the PS (:174).
   MF_ONLINE_SPARK_SWEEP emits only touched rows (OfflineSpark.scala:33-67): outputs must be NULL. */
int mf_online_update_out(mf_ctx* ctx, const int32_t* users, const int32_t* items,
                         const double* ratings, int64_t n, int flavour, int num_partitions,
                         int64_t* touched_users, int64_t* touched_items, double* user_out,
                         double* item_out);
/* Online updates on implicit feedback: every event is followed by `negatives` sampled updates
   (users[j], another item, negative_rating), drawn and expanded on the device.
   Meaning.  The call is mf_online_update(flavour, arrival order) on the expanded batch, bit for bit: N =
   n * (1 + negatives) records, for each event j its own (users[j], items[j], ratings[j]) followed by
   (users[j], id of row_{j,s}, negative_rating) for s = 0 .. negatives-1.  Only the events bring new ids;
   they get rows and first-touch values exactly as mf_online_update gives them, before anything is drawn.
   touched_* and mf_stats.updates count the expanded batch.
   The draw.  Event j of the call is event t = first_event + j of the stream.  With pool = the item rows
   the model holds once this batch's new ids have theirs and pos_row = the factor row of items[j]:
       z = (uint64)seed + 0x9E3779B97F4A7C15 * (t * 64 + s + 1)     (mod 2^64: SplitMix64)
       z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z ^= z >> 31
       c = ((z >> 32) * (pool - 1)) >> 32;        row = c + (c >= pos_row)
   uniform over the other pool - 1 rows, never the event's own item; no rejection, duplicates among one
   event's negatives allowed.  A batch that leaves the model with one item (pool == 1) has nothing to
   draw from: the call is then mf_online_update on the events alone and sampled_items_out is not written.
   The pool is indexed by factor row (rows are given in first-touch order), so the draws of a given (seed,
   first_event) depend on the model's row layout: they are reproducible for the same sequence of calls on
   the same model, not across models built in another order.  The library keeps no counter: the caller
   passes first_event and advances it by n, so a checkpointed stream resumes exactly.
   sampled_items_out (may be NULL) receives the n * negatives drawn item ids, event-major; they are mapped
   from rows on the host only when asked for.  mf_negative_draws is the draw itself (rows, no GPU needed).
   Errors: mf_online_update's own; MF_ERR_INVALID for negatives outside 0 .. MF_NEG_MAX, a negative_rating
   that is not finite, first_event < 0, N >= 2^31, or flavour == MF_ONLINE_SPARK_SWEEP (its sequence is not
   the arrival order).  negatives == 0 is exactly mf_online_update; n == 0 is valid.  Validation runs
   before anything is inserted or updated. */
#define MF_NEG_MAX 64
int mf_online_update_sampled(mf_ctx* ctx, const int32_t* users, const int32_t* items, const double* ratings,
                             int64_t n, int flavour, int32_t negatives, double negative_rating,
                             int64_t seed, int64_t first_event,
                             int32_t* sampled_items_out /* [n * negatives] item ids, or NULL */,
                             int64_t* touched_users, int64_t* touched_items);
/* rows_out[j * negatives + s] = the draw above for event first_event + j with pos_row[j] < pool.
   MF_ERR_INVALID: n < 0, negatives outside 0 .. MF_NEG_MAX, first_event < 0, pool outside 1 .. 2^31, a
   pos_row outside the pool, or pool == 1 with something to draw. */
int mf_negative_draws(int64_t seed, int64_t first_event, int64_t n, int32_t negatives, int64_t pool,
                      const int32_t* pos_row /* [n] */, int32_t* rows_out /* [n * negatives] */);
/* mf_online_prequential with mf_online_update_sampled as its step 2.  Step 1 is unchanged: it ranks the n
   events against the model on entry.  Errors: mf_online_prequential's and mf_online_update_sampled's. */
int mf_online_prequential_sampled(mf_ctx* ctx, const int32_t* users, const int32_t* items, const double* ratings,
                                  int64_t n, int flavour, int32_t top_n,
                                  const int32_t* excl_user, const int32_t* excl_item, int64_t n_excl,
                                  mf_prequential* out, int32_t* rank_out /* [n] or NULL */,
                                  int64_t* touched_users, int64_t* touched_items,
                                  int32_t negatives, double negative_rating, int64_t seed, int64_t first_event,
                                  int32_t* sampled_items_out /* [n * negatives] or NULL */);
/* The resident seen set: the distinct (user, item) pairs the model's readers hide ("filter already seen"),
   built once and kept on the device keyed by factor row, so that the four calls below name it instead of
   passing -- and resolving, uploading and sorting -- the same exclusion arrays in every call.
   mf_seen_set replaces the set with the distinct pairs given; n == 0 leaves an empty set.  mf_seen_add forms
   the union with what is held (only the batch is sorted; on a context with no set it is mf_seen_set).  A
   pair naming a user or item id the model does not hold at the time of the call is dropped, mf_recommend's
   rule for exclusion pairs, and counted in *ignored_out (may be NULL); duplicates count once.
   mf_seen_from_als replaces the set with the distinct (user, item) pairs of the data mf_als_prepare /
   mf_als_append left on the device: nothing is uploaded, ratings of every sign count (a rated pair is a seen
   pair).  It is a snapshot: a later mf_als_append does not change the set, the caller follows it with
   mf_seen_add of the same batch.  mf_seen_clear leaves no set; mf_seen_count gives the distinct pairs held
   (64-bit; 0 with no set).
   mf_seen_remove is the set difference: the set becomes the held set minus the pairs given.  *removed_out
   (may be NULL) is the number of distinct pairs that were held and are gone, *ignored_out (may be NULL) the
   pairs naming an unknown id, mf_seen_add's rule.  Pairs that are not held are no error.  With no set the call
   changes nothing and still writes both outputs (*removed_out = 0).  Errors and state rules are mf_seen_add's.
   The set has no multiplicity: after mf_als_remove on a window in which a pair may recur, the exact seen set
   is mf_seen_from_als again, not mf_seen_remove of the expired batch.
   Lifetime.  The set survives everything that only adds rows -- mf_online_update*, mf_set_factors,
   mf_load_model, mf_als_append, every run call -- and a row gained after the set was built has no seen pairs
   until some are added.  mf_dsgd_prepare / mf_dsgd_fit rebuild the rows and leave no set, as they invalidate
   the ALS data.  The set is not part of mf_save_model.
   Readers.  mf_recommend_seen, mf_rank_eval_seen and mf_pair_ranks_seen return, bit for bit, what
   mf_recommend, mf_rank_eval and mf_pair_ranks return when given every pair of the set as excl_* arrays: ids,
   scores, counts, ranks, codes, valid_out, every metric and sum, under all of their rules ("a pair both
   excluded and in the ground truth stays in G and is never hit" among them).  Both query sides work: user
   queries exclude items, item queries users (that orientation of the table is made from the other on first
   use and kept until the set changes; it needs a set of fewer than 2^31 - 1 pairs).  No set, or an empty one,
   is n_excl == 0.  mf_online_prequential_seen is mf_online_prequential_sampled with the set as its
   exclusions (negatives == 0: mf_online_prequential for the two arrival-order flavours;
   MF_ONLINE_SPARK_SWEEP is refused as there); with add_events != 0 it ends with mf_seen_add(users, items,
   n), when every id of the batch is known, so that the next batch's events find these seen: the prequential
   loop a caller would otherwise write by hand.
   Errors.  MF_ERR_INVALID: a NULL context, a negative count, a NULL array with a positive count, n >= 2^31 -
   1 pairs in one call (mf_seen_from_als: as many ratings in the prepared data), and whatever the namesake
   refuses.  MF_ERR_STATE: every call here on a rank-mode context; mf_seen_from_als wherever mf_als_run would
   fail for want of prepared data.  MF_ERR_NOT_FITTED from the three readers as from their namesakes.  All
   validation runs before anything changes.  A context on several devices keeps the set on its first. */
int mf_seen_set(mf_ctx* ctx, const int32_t* users, const int32_t* items, int64_t n, int64_t* ignored_out);
int mf_seen_add(mf_ctx* ctx, const int32_t* users, const int32_t* items, int64_t n, int64_t* ignored_out);
int mf_seen_remove(mf_ctx* ctx, const int32_t* users, const int32_t* items, int64_t n, int64_t* removed_out,
                   int64_t* ignored_out);
int mf_seen_from_als(mf_ctx* ctx);
int mf_seen_clear(mf_ctx* ctx);
int mf_seen_count(mf_ctx* ctx, int64_t* pairs);
int mf_recommend_seen(mf_ctx* ctx, int query_side, const int32_t* queries, int64_t n_queries, int32_t top_n,
                      int32_t* ids_out, double* scores_out, int32_t* counts_out);
int mf_rank_eval_seen(mf_ctx* ctx, int query_side,
                      const int32_t* gt_query, const int32_t* gt_cand, int64_t n_gt,
                      int32_t top_n, mf_rank_metrics* out,
                      int32_t* q_ids_out, int32_t* q_counts_out, double* q_metrics_out, int64_t cap);
int mf_pair_ranks_seen(mf_ctx* ctx, int query_side,
                       const int32_t* queries, const int32_t* cands, int64_t n,
                       int32_t* rank_out, int32_t* valid_out /* or NULL */, double* score_out /* or NULL */);
int mf_online_prequential_seen(mf_ctx* ctx, const int32_t* users, const int32_t* items, const double* ratings,
                               int64_t n, int flavour, int32_t top_n,
                               mf_prequential* out, int32_t* rank_out /* [n] or NULL */,
                               int64_t* touched_users, int64_t* touched_items,
                               int32_t negatives, double negative_rating, int64_t seed, int64_t first_event,
                               int32_t* sampled_items_out /* [n * negatives] or NULL */,
                               int add_events);
/* BPR ranking training (Bayesian personalised ranking, Rendle et al. 2009) on the resident seen set, as
   synchronous minibatches.  A step takes `batch` slots; a slot is a triple (user row u, positive item row i,
   negative item row j) or void.  Every gradient of a step is taken from the model as the step found it, and
   every touched row is written once, from a sum taken in a fixed order: no floating-point atomics, and the
   result is defined operation by operation below, so that it can be replayed bit for bit (mfhip/bpr.py).
   T is float on a fast context and double on a deterministic one; lr and lambda are rounded to T once.

   The draw (mf_bpr_run).  The table is the seen set's user-major one: per user factor row its distinct item
   rows, ascending, `pairs` entries in all, entry e belonging to the row with off[row] <= e < off[row + 1];
   pool = the item rows the model holds.  Draw r of slot s of step t:
       z = (uint64)seed + 0x9E3779B97F4A7C15 * (t * 2^38 + s * 64 + r + 1)   (mod 2^64),
   then the SplitMix64 finaliser of mf_online_update_sampled.  r = 0 is the positive: entry e = (z * pairs) >>
   64 of the table, u = its row, i = the entry.  r = 1 .. 1 + redraws are negatives: c = ((z >> 32) * (pool -
   1)) >> 32, row = c + (c >= i); the first one that u's table row does not hold is j.  If u holds all of them
   the slot is void; with pool == 1 or an empty set every slot is void.  A draw depends on (seed, t, s, r) and
   the table alone, not on the batch size or any other slot.  The library keeps no counter: the caller advances
   first_step, as first_event of mf_online_update_sampled.  mf_bpr_draws gives, with no GPU, z_out[s * (2 +
   redraws) + 0] = e and z_out[s * (2 + redraws) + r] = c of draw r >= 1 (pairs == 0: e = 0; pool == 1: c = 0).

   One step.  All reads see the model as the step found it.  No operation is fused: every product is rounded
   before it is added.
   1. d[f] = q_i[f] - q_j[f].
   2. x = p_u . d in 64 partials: partial l is the chain ((0 + p[l] d[l]) + p[l + 64] d[l + 64]) + ... over f = l,
      l + 64, l + 128, l + 192 below k (0 if there is none); the partials are then added pairwise, v[l] = v[l] +
      v[l ^ 32] for every l at once, then the same with 16, 8, 4, 2, 1; x = v[0].  (k <= 256.)
   3. g = T(1 / (1 + E(x))) with x widened to f64 and E(x) evaluated in f64: a NaN stays; x is clamped to [-40,
      40]; n = rint(x * 1.4426950408889634); r = (x - n * 6.93147180369123816490e-01) - n *
      1.90821492927058770002e-10; P = the polynomial sum_{i <= 13} r^i / i! by Horner's rule from the coefficient
      1 / 13! down, each step one multiplication and one addition, the coefficients being the f64 quotients 1.0 /
      i!; E = ldexp(P, n).  Measured against numpy.exp on [-40, 40]: a largest relative difference of 2.22e-16.
   4. User row a, over its non-void slots in ascending s (n_a of them): per factor a chain from 0, acc = acc +
      g_s * d_s[f].  A segment of more than 1,024 slots takes one such chain per 1,024 consecutive slots of it
      and then adds the chain results to 0 in ascending order.  With c = 1, m = n_a (MF_BPR_SCALE_SUM) or c =
      T(1) / T(n_a), m = 1 (MF_BPR_SCALE_MEAN): p'[f] = p[f] + lr * (c * acc[f] - (lambda * T(m)) * p[f]), lambda *
      T(m) rounded once, then the two products, the difference, the product with lr, and the sum.
   5. Item row b the same, over its entries in ascending (s, positive before negative): + g_s * p_u[f] where b is
      slot s's positive, - g_s * p_u[f] (the product subtracted) where it is its negative; n_b counts both kinds.
   6. Both sides are computed from the model as the step found it; neither sees the other's new rows.

   Scale rules.  SUM is the textbook sum of per-triple steps and suits batches in which a row gathers a few
   slots per step (up to a few thousand slots on 10^2 .. 10^3 rows, any batch on a large catalogue); its step
   grows with a row's count, and at ~100 slots per row (lr 0.05) the factors overflow.  MEAN divides a row's
   step by its count, so it holds for any batch, with a learning rate about ten times SUM's.

   mf_bpr_run runs steps first_step .. first_step + steps - 1, queued with no host synchronisation between
   them; *out (may be NULL) receives the counts summed over the call: slots = steps * batch, the void ones, and
   the rows written per side (a row counts once per step that writes it).  mf_bpr_step_triples runs one step on
   n caller-given triples of ids (n <= 2^24), resolved on the device: a triple naming an unknown id or with
   pos == neg is void, counted and with no other effect; batch, redraws and seed are not read.  mf_bpr_fit
   gives the unseen ids of the n pairs rows under mf_als_prepare's insertion rules, their initial values
   multiplied by init_scale in f64 before the rounding to T (rows already held are kept), then is
   mf_seen_set(users, items, n) and mf_bpr_run(first_step = 0).
   State.  Single device, single process: MF_ERR_STATE on a rank-mode or multi-device context, and from
   mf_bpr_run without a seen set.  MF_ERR_NOT_FITTED from mf_bpr_step_triples on a context with no model.
   MF_ERR_INVALID: a NULL context or params, a NULL array with a positive count, lr not finite or <= 0, lambda
   not finite or < 0, an unknown scale, batch outside 1 .. 2^24, redraws outside 0 .. 62, a negative count or
   step, a step at or past 2^26, k > 256, init_scale not finite.  All validation runs before anything changes.
   The seen set, the ALS data and its half-sweep counter, a prepared DSGD schedule and mf_als_nonneg_stats
   stay untouched by mf_bpr_run and mf_bpr_step_triples, and rows that no non-void slot names keep their bits. */
#define MF_BPR_SCALE_SUM  0
#define MF_BPR_SCALE_MEAN 1
typedef struct mf_bpr_params {
  double lr, lambda;
  int32_t batch;      /* slots per step, 1 .. 2^24 */
  int32_t scale;      /* MF_BPR_SCALE_* */
  int32_t redraws;    /* 0 .. 62: further draws of a negative the user has seen */
  int32_t reserved0;
  int64_t seed;
  int32_t reserved[4];
} mf_bpr_params;
typedef struct mf_bpr_stats { int64_t slots, void_slots, user_rows_written, item_rows_written; } mf_bpr_stats;
int mf_bpr_run(mf_ctx* ctx, const mf_bpr_params* params, int64_t first_step, int64_t steps,
               mf_bpr_stats* out /* or NULL */);
int mf_bpr_step_triples(mf_ctx* ctx, const mf_bpr_params* params, const int32_t* users, const int32_t* pos_items,
                        const int32_t* neg_items, int64_t n, mf_bpr_stats* out /* or NULL */);
int mf_bpr_draws(int64_t seed, int64_t step, int32_t batch, int32_t redraws, int64_t pairs, int64_t pool,
                 uint64_t* z_out /* batch x (2 + redraws) */);
int mf_bpr_fit(mf_ctx* ctx, const int32_t* users, const int32_t* items, int64_t n, double init_scale,
               const mf_bpr_params* params, int64_t steps, mf_bpr_stats* out /* or NULL */);
/* Vectors for specific ids (found[j] = 0 for unknown ids). */
int mf_lookup(mf_ctx* ctx, int side, const int32_t* ids, int64_t n, double* vecs_out,
              uint8_t* found);

/* Statistics; profiling = 1 times every sweep-kernel launch with HIP events. */
int mf_set_profiling(mf_ctx* ctx, int on);
int mf_get_stats(mf_ctx* ctx, mf_stats* out);
int mf_reset_stats(mf_ctx* ctx);

/* JVM-compatible helpers used by the shim and tests (no GPU needed). */
int mf_jvm_shuffle(int64_t seed, int64_t len, int32_t* out);           /* scala.util.Random.shuffle */
int mf_jvm_block_of(int32_t id, int64_t seed, int32_t n_blocks, int32_t* out);  /* :531-533 */
int mf_jvm_random_factors(int64_t rng_seed, int32_t k, double* out);   /* k x nextDouble */
int mf_learning_rate(int method, double lr, int32_t iteration, double lambda, double arg,
                     double* out);

#ifdef __cplusplus
}
#endif
#endif /* MFHIP_H */
