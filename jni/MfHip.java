// MfHip.java -- JNI entry points of libmfhip.so for the reference's Scala jobs (INTEGRATION.md).
// Goes to core/src/main/java/hu/sztaki/ilab/recom/core/gpu/MfHip.java in the reference tree; the
// native side is jni/mfhip_jni.c.  Every native method throws RuntimeException on a non-zero
// status, carrying mf_last_error() (MatrixFactorization.scala:189-190, 270-271 throw the same).
package hu.sztaki.ilab.recom.core.gpu;

public final class MfHip {
  static { System.loadLibrary("mfhipjni"); }   // links libmfhip.so

  public static final int MODE_DETERMINISTIC_F64 = 0, MODE_FAST_F32 = 1;
  // flink-ml LearningRateMethod (DSGDforMF.scala:10, 167-169)
  public static final int LR_DEFAULT = 0, LR_CONSTANT = 1, LR_BOTTOU = 2, LR_INVSCALING = 3, LR_XU = 4;
  public static final int SIDE_USER = 0, SIDE_ITEM = 1;
  public static final int ONLINE_NEXT_FACTORS = 0, ONLINE_DELTA = 1, ONLINE_SPARK_SWEEP = 2;
  public static final int INIT_PSEUDO_RANDOM = 0, INIT_SEEDED = 1;
  public static final int UID_BYTES = 128;

  // mf_create: params as MatrixFactorization.scala:201-223 / DSGDforMF.scala:163-169
  public static native long create(int k, int iterations, double lambda, double lr, int lrMethod,
                                   double lrArg, int numBlocks, long seed, boolean hasSeed, int mode,
                                   double onlineLr, int onlineInit, int[] deviceIds);
  // mf_comm_unique_id / mf_create_rank: one task per GPU, the id shipped by a broadcast variable
  public static native byte[] commUniqueId();
  public static native long createRank(int k, int iterations, double lambda, double lr, int lrMethod,
                                       double lrArg, int numBlocks, long seed, boolean hasSeed, int mode,
                                       int deviceId, int nranks, int rank, byte[] uid);
  public static native void destroy(long ctx);
  // fitSGD.fit (DSGDforMF.scala:262-357) in one call, or staged: prepare (blocking, :279-337),
  // run supersteps (the BulkIteration, :341-344), restart from the initial factors, sync
  public static native void dsgdFit(long ctx, int[] users, int[] items, double[] ratings);
  public static native void dsgdPrepare(long ctx, int[] users, int[] items, double[] ratings);
  public static native void dsgdRun(long ctx, long supersteps);
  public static native void dsgdRestart(long ctx);
  public static native void sync(long ctx);
  // ALS.train(ratings, rank = numFactors, iterations, lambda) (OnlineSpark.scala:125-131);
  // reg: 0 = lambda * n_row (ALS-WR, what ALS.train does), 1 = plain lambda
  public static native void alsFit(long ctx, int[] users, int[] items, double[] ratings,
                                   int iterations, double lambda, int reg);
  // ALS.trainImplicit(ratings, rank = numFactors, iterations, lambda, alpha): confidences
  // 1 + alpha |r|, preferences r > 0; reg as above, with n_row counting the ratings r > 0
  public static native void alsFitImplicit(long ctx, int[] users, int[] items, double[] ratings,
                                           int iterations, double lambda, int reg, double alpha);
  // The same half-sweeps by conjugate gradients (mf_als_fit_cg / mf_als_fit_implicit_cg): cgSteps
  // (1..256) CG steps per row from its current value instead of a factorisation.  alsPrepare
  // (mf_als_prepare) keeps the ratings on the device; alsRunCg / alsRunImplicitCg then run half-sweeps
  // (item side first, one counter shared by every kind of run call).
  public static native void alsPrepare(long ctx, int[] users, int[] items, double[] ratings);
  public static native void alsFitCg(long ctx, int[] users, int[] items, double[] ratings,
                                     int iterations, double lambda, int reg, int cgSteps);
  public static native void alsFitImplicitCg(long ctx, int[] users, int[] items, double[] ratings,
                                             int iterations, double lambda, int reg, double alpha, int cgSteps);
  public static native void alsRunCg(long ctx, long halfSweeps, double lambda, int reg, int cgSteps);
  public static native void alsRunImplicitCg(long ctx, long halfSweeps, double lambda, int reg, double alpha,
                                             int cgSteps);
  // Non-negative ALS (MLlib's nonnegative = true; mf_als_fit_nonneg / mf_als_fit_implicit_nonneg): every row
  // is solved for x >= 0 by a projected conjugate-gradient NNLS.  The run calls follow alsPrepare and share
  // the half-sweep counter with every other kind of run call.
  public static native void alsFitNonneg(long ctx, int[] users, int[] items, double[] ratings,
                                         int iterations, double lambda, int reg);
  public static native void alsFitImplicitNonneg(long ctx, int[] users, int[] items, double[] ratings,
                                                 int iterations, double lambda, int reg, double alpha);
  public static native void alsRunNonneg(long ctx, long halfSweeps, double lambda, int reg);
  public static native void alsRunImplicitNonneg(long ctx, long halfSweeps, double lambda, int reg, double alpha);
  // Incremental ALS (mf_als_append / mf_als_run_rows / mf_als_update), after alsPrepare or an alsFit*: the
  // ratings join the CSRs on the device, and only named rows are solved.  The half-sweep is named by lambda,
  // reg, implicit (0 / 1, alpha read only then), solver (0 Cholesky, 1 CG with cgSteps, 2 NNLS).
  // alsRunRows returns the rows solved.  alsUpdate appends, then `rounds` times solves the batch's users and
  // then its items -- users first, unlike a full sweep: a new user's row is random until it is solved;
  // solvedOut (may be null, length >= 2) receives the last round's user and item counts.
  public static native void alsAppend(long ctx, int[] users, int[] items, double[] ratings);
  public static native long alsRunRows(long ctx, int side, int[] ids, double lambda, int reg, int implicit,
                                       double alpha, int solver, int cgSteps);
  public static native void alsUpdate(long ctx, int[] users, int[] items, double[] ratings, double lambda,
                                      int reg, int implicit, double alpha, int solver, int cgSteps, int rounds,
                                      int[] solvedOut);
  // The objective the half-sweeps minimise (mf_als_objective), on the resident data at the factors as they
  // stand; nothing is uploaded and nothing changes.  Returns total; lossOut (may be null, length >= 8) receives
  // total, fit, unobserved, reg_user, reg_item, ratings, user_rows, item_rows.  alsRunUntil (mf_als_run_until)
  // runs iterations of two half-sweeps until one lowers the objective by no more than relTol times its size, at
  // most maxIterations; returns the iterations taken; historyOut (may be null, length >= maxIterations + 1)
  // receives the objective on entry and after every iteration.
  public static native double alsObjective(long ctx, double lambda, int reg, int implicit, double alpha,
                                           double[] lossOut);
  public static native int alsRunUntil(long ctx, double lambda, int reg, int implicit, double alpha, int solver,
                                       int cgSteps, int maxIterations, double relTol, double[] historyOut);
  // Removal (mf_als_remove / mf_als_remove_rows / mf_als_retract): entry j removes the oldest rating of the
  // pair (users[j], items[j]) still held; alsRemoveRows removes every rating of the named users or items (the
  // factor rows stay); alsRetract removes, then `rounds` times solves the batch's users and then its items.
  // Each returns the ratings removed; foundOut (may be null, length >= n) receives 0 / 1 per entry, solvedOut
  // (may be null, length >= 2) the last round's user and item counts.
  public static native long alsRemove(long ctx, int[] users, int[] items, byte[] foundOut);
  public static native long alsRemoveRows(long ctx, int side, int[] ids);
  public static native long alsRetract(long ctx, int[] users, int[] items, double lambda, int reg, int implicit,
                                       double alpha, int solver, int cgSteps, int rounds, byte[] foundOut,
                                       int[] solvedOut);
  // unblock (DSGDforMF.scala:245-255) and checkpoint restore
  public static native long numFactors(long ctx, int side);
  public static native long getFactors(long ctx, int side, int[] idsOut, double[] vecsOut);
  public static native void setFactors(long ctx, int side, int[] ids, double[] vecs);
  // predictRating / RMSE / empiricalRisk (MatrixFactorization.scala:133-192, 239-274)
  public static native void predict(long ctx, int[] users, int[] items, double[] out, byte[] found);
  public static native double rmse(long ctx, int[] users, int[] items, double[] r);
  public static native double empiricalRisk(long ctx, int[] users, int[] items, double[] r, double lambda);
  // MatrixFactorizationModel.recommendProducts / recommendUsers / recommendProductsForUsers:
  // idsOut / scoresOut (may be null) hold queries.length * topN entries, countsOut queries.length;
  // exclQuery / exclCand (both null, or equal lengths) are pairs never returned
  public static native void recommend(long ctx, int querySide, int[] queries, int topN,
                                      int[] exclQuery, int[] exclCand,
                                      int[] idsOut, double[] scoresOut, int[] countsOut);
  // nearest neighbours in factor space (mf_similar, mf_recommend_vectors); outputs as for recommend
  public static final int METRIC_DOT = 0, METRIC_COSINE = 1;
  // for every queries[j] (an id of `side`) the topN nearest ids of the same side; the query's own row is
  // left out unless includeSelf
  public static native void similar(long ctx, int side, int[] queries, int topN, int metric, boolean includeSelf,
                                    int[] exclQuery, int[] exclCand,
                                    int[] idsOut, double[] scoresOut, int[] countsOut);
  // the topN rows of candSide for numQueries vectors the model need not hold (vecs: numQueries * k doubles,
  // row-major); exclQueryIndex[e] names a position in vecs
  public static native void recommendVectors(long ctx, int candSide, double[] vecs, int numQueries, int topN,
                                             int metric, int[] exclQueryIndex, int[] exclCand,
                                             int[] idsOut, double[] scoresOut, int[] countsOut);
  // the topN among caller-given candidate ids only (mf_recommend_among); outputs as for recommend.  offsets
  // null: every query ranks the one list candIds (an allow-list); otherwise query j ranks entries offsets[j] ..
  // offsets[j + 1] of candIds (queries.length + 1 entries from 0 to candIds.length, not decreasing).  Ids the
  // model does not hold are dropped, repeated ids count once.  excludeSeen: the resident seen set is the
  // exclusion list and exclQuery / exclCand must be null
  public static native void recommendAmong(long ctx, int querySide, int[] queries, int topN, int[] offsets,
                                           int[] candIds, boolean excludeSeen, int[] exclQuery, int[] exclCand,
                                           int[] idsOut, double[] scoresOut, int[] countsOut);
  // Fold-in (mf_als_foldin / mf_recommend_foldin): vectors for users (side 0; the lists name items) or items
  // (side 1; the lists name users) the model does not hold and does not take in -- nothing of the context
  // changes.  Query j owns entries offsets[j] .. offsets[j + 1] of candIds / ratings (offsets: numQueries + 1
  // entries from 0, not decreasing); ids the model does not hold are dropped; the solve is named as for
  // alsRunRows.  vecsOut: numQueries * k doubles; usedOut (may be null, one entry per query): the kept entries.
  // recommendFoldin scores the vectors on the device like recommendVectors with the dot product; with
  // excludeRated a query's kept ids are never returned to it; a query with no kept entry has count 0;
  // vecsOut may be null there.
  public static native void alsFoldin(long ctx, int side, int[] offsets, int[] candIds, double[] ratings,
                                      double lambda, int reg, int implicit, double alpha, int solver, int cgSteps,
                                      double[] vecsOut, int[] usedOut);
  public static native void recommendFoldin(long ctx, int side, int[] offsets, int[] candIds, double[] ratings,
                                            double lambda, int reg, int implicit, double alpha, int solver,
                                            int cgSteps, int topN, boolean excludeRated,
                                            int[] idsOut, double[] scoresOut, int[] countsOut,
                                            double[] vecsOut, int[] usedOut);
  // RankingMetrics of held-out (query, candidate) pairs against the model's topN lists (mf_rank_eval),
  // taken on the device.  metricsOut (length >= 8) receives queries, hits, precision, recall, MAP, NDCG,
  // MRR, hit rate; exclQuery / exclCand as for recommend
  public static native void rankEval(long ctx, int querySide, int[] gtQuery, int[] gtCand, int topN,
                                     int[] exclQuery, int[] exclCand, double[] metricsOut);
  // the 0-based position of every (queries[j], cands[j]) in the query's complete ranked list (mf_pair_ranks):
  // ranksOut[j] = -1 for an id the model does not hold, -2 for a pair in the exclusion list; validOut
  // (may be null) the length of the list, scoresOut (may be null) the pair's score as recommend reports it
  public static native void pairRanks(long ctx, int querySide, int[] queries, int[] cands,
                                      int[] exclQuery, int[] exclCand, int[] ranksOut, int[] validOut,
                                      double[] scoresOut);
  // prequential evaluation of one micro-batch (mf_online_prequential): every event is ranked against the
  // model as it stands, then onlineUpdate(users, items, r, flavour, numPartitions) runs.  metricsOut
  // (length >= 12) receives events, evaluated, cold, excluded, hits, the sums of NDCG, RR and percentile
  // rank, then NDCG, MRR, hit rate and mean percentile rank; ranksOut (may be null) every event's rank
  public static native void onlinePrequential(long ctx, int[] users, int[] items, double[] r,
                                              int flavour, int numPartitions, int topN,
                                              int[] exclUser, int[] exclItem, double[] metricsOut, int[] ranksOut);
  // implicit feedback (mf_online_update_sampled / mf_online_prequential_sampled): every event is followed
  // by `negatives` (0 .. 64) updates (user, another item drawn on the device, negRating).  firstEvent: the
  // events of the stream before this batch -- the caller adds users.length after every call.  sampledOut
  // (may be null, length >= users.length * negatives) receives the drawn item ids, event-major.
  public static native void onlineUpdateSampled(long ctx, int[] users, int[] items, double[] r, int flavour,
                                                int negatives, double negRating, long seed, long firstEvent,
                                                int[] sampledOut);
  public static native void onlinePrequentialSampled(long ctx, int[] users, int[] items, double[] r,
                                                     int flavour, int topN, int[] exclUser, int[] exclItem,
                                                     double[] metricsOut, int[] ranksOut, int negatives,
                                                     double negRating, long seed, long firstEvent,
                                                     int[] sampledOut);
  // the resident seen set (mf_seen_*): the distinct (user, item) pairs the readers hide, kept on the device.
  // seenSet replaces it, seenAdd forms the union (both return the pairs ignored for an unknown id),
  // seenFromAls takes the pairs of the prepared ALS data without an upload.  The four *Seen readers are
  // recommend / rankEval / pairRanks / onlinePrequentialSampled with the set as their exclusions, bit for
  // bit; addEvents: the batch joins the set after the update
  public static native long seenSet(long ctx, int[] users, int[] items);
  public static native long seenAdd(long ctx, int[] users, int[] items);
  // seenRemove (mf_seen_remove): the set minus the pairs given; returns the distinct held pairs removed,
  // ignoredOut (may be null, length >= 1) receives the pairs naming an unknown id
  public static native long seenRemove(long ctx, int[] users, int[] items, int[] ignoredOut);
  public static native void seenFromAls(long ctx);
  public static native void seenClear(long ctx);
  public static native long seenCount(long ctx);
  public static native void recommendSeen(long ctx, int querySide, int[] queries, int topN,
                                          int[] idsOut, double[] scoresOut, int[] countsOut);
  public static native void rankEvalSeen(long ctx, int querySide, int[] gtQuery, int[] gtCand, int topN,
                                         double[] metricsOut);
  public static native void pairRanksSeen(long ctx, int querySide, int[] queries, int[] cands,
                                          int[] ranksOut, int[] validOut, double[] scoresOut);
  public static native void onlinePrequentialSeen(long ctx, int[] users, int[] items, double[] r,
                                                  int flavour, int topN, double[] metricsOut, int[] ranksOut,
                                                  int negatives, double negRating, long seed, long firstEvent,
                                                  int[] sampledOut, boolean addEvents);
  // BPR ranking training on the seen set (mf_bpr_run / mf_bpr_step_triples / mf_bpr_fit): synchronous minibatch
  // steps, positives drawn from the set and negatives checked against it on the device.  scale: 0 = sum of the
  // slots' steps per row, 1 = their mean.  The caller advances firstStep.  statsOut (may be null, length >= 4):
  // slots, void slots, user rows written, item rows written
  public static native void bprRun(long ctx, double lr, double lambda, int batch, int scale, int redraws, long seed,
                                   long firstStep, long steps, double[] statsOut);
  public static native void bprStepTriples(long ctx, double lr, double lambda, int scale, int[] users,
                                           int[] posItems, int[] negItems, double[] statsOut);
  public static native void bprFit(long ctx, int[] users, int[] items, double initScale, double lr, double lambda,
                                   int batch, int scale, int redraws, long seed, long steps, double[] statsOut);
  public static native void blockUpdate(long ctx, double[] r, int[] uidx, int[] iidx,
                                        double[] users, int[] uomega, double[] items, int[] iomega,
                                        int k, int iteration, int ratingBlockId, long seed,
                                        double lr, int lrMethod, double lrArg, double lambda);
  // online micro-batches; onlineUpdateOut also returns every rating's emitted vectors
  // (FlinkOnlineMF.scala:131-135 / PSOfflineOnlineMF.scala:174-176), n x k each (may be null)
  public static native void onlineUpdate(long ctx, int[] users, int[] items, double[] r,
                                         int flavour, int numPartitions);
  public static native void onlineUpdateOut(long ctx, int[] users, int[] items, double[] r,
                                            int flavour, double[] userOut, double[] itemOut);
  public static native void lookup(long ctx, int side, int[] ids, double[] vecsOut, byte[] found);
  // env.readCsvFile[(Int, Int, Double)] replacement (DSGDforMF.scala:72)
  public static native long countRatings(String path, char delimiter, int skipLines);
  public static native void readRatings(String path, char delimiter, int skipLines, int[] users,
                                        int[] items, double[] ratings);
  // TemporaryPath persistence of the fit; loadModel returns the superstep counter
  public static native void saveModel(long ctx, String path);
  public static native long loadModel(long ctx, String path);
}
