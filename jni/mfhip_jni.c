/*
 * mfhip_jni.c -- the JNI shim behind jni/MfHip.java.  Goes to
 * core/src/main/native/ in the reference tree; links libmfhip.so:
 *   gcc -O2 -shared -fPIC -I$JAVA_HOME/include -I$JAVA_HOME/include/linux -I<repo>/include \
 *       mfhip_jni.c -L<repo>/large-scale-recommendation_amd/lib -lmfhip -Wl,-rpath,'$ORIGIN' \
 *       -o libmfhipjni.so
 * Every non-zero status becomes a java.lang.RuntimeException carrying mf_last_error(), which is
 * what the reference throws for the same conditions (MatrixFactorization.scala:189-190, 270-271).
 * Array lengths are checked against what the C call reads or writes BEFORE any element is
 * touched (IllegalArgumentException, as the reference's argument checks).  Arrays cross with
 * Get<Type>ArrayElements / Release<Type>ArrayElements, never as JNI critical regions: a fit or a
 * micro-batch runs for seconds, and a critical region held that long would stall the garbage
 * collector of every Flink/Spark task thread.  (The library never retains host pointers.)
 * tests/test_abi.py compiles this file against include/mfhip.h (with a minimal jni.h stand-in,
 * this image has no JDK) so every call matches the C ABI.
 */
#include <jni.h>
#include <stdint.h>
#include <stdlib.h>

#include "mfhip.h"

static void throw_named(JNIEnv* env, const char* cls, const char* msg) {
  jclass ex = (*env)->FindClass(env, cls);
  if (ex) (*env)->ThrowNew(env, ex, msg);
}

static int check(JNIEnv* env, int st) {
  if (st != MF_OK) throw_named(env, "java/lang/RuntimeException", mf_last_error());
  return st;
}

/* 0 when ok; otherwise an IllegalArgumentException is pending. */
static int require(JNIEnv* env, int ok, const char* msg) {
  if (!ok) throw_named(env, "java/lang/IllegalArgumentException", msg);
  return ok ? 0 : -1;
}

static jsize len(JNIEnv* env, jarray a) { return a ? (*env)->GetArrayLength(env, a) : 0; }

/* Element access by copy (or by the VM's choice, never a critical region). */
enum { kInt, kDouble, kByte };
typedef struct {
  jarray a;
  void* p;
  int kind;
} Elems;

static int acquire(JNIEnv* env, Elems* e, jarray a, int kind) {
  e->a = a;
  e->kind = kind;
  e->p = NULL;
  if (!a) return 0;
  switch (kind) {
    case kInt: e->p = (*env)->GetIntArrayElements(env, (jintArray)a, NULL); break;
    case kDouble: e->p = (*env)->GetDoubleArrayElements(env, (jdoubleArray)a, NULL); break;
    default: e->p = (*env)->GetByteArrayElements(env, (jbyteArray)a, NULL); break;
  }
  return e->p ? 0 : -1; /* NULL: OutOfMemoryError is pending */
}

/* mode 0: copy back (outputs), JNI_ABORT: discard (inputs). */
static void release(JNIEnv* env, Elems* e, jint mode) {
  if (!e->a || !e->p) return;
  switch (e->kind) {
    case kInt: (*env)->ReleaseIntArrayElements(env, (jintArray)e->a, (jint*)e->p, mode); break;
    case kDouble: (*env)->ReleaseDoubleArrayElements(env, (jdoubleArray)e->a, (jdouble*)e->p, mode); break;
    default: (*env)->ReleaseByteArrayElements(env, (jbyteArray)e->a, (jbyte*)e->p, mode); break;
  }
  e->p = NULL;
}

#define JFN(name) Java_hu_sztaki_ilab_recom_core_gpu_MfHip_##name
#define CTX(h) ((mf_ctx*)(intptr_t)(h))

/* The context's rank k (row length of every factor buffer), or -1 with an exception pending. */
static jlong rank_of(JNIEnv* env, jlong h) {
  mf_params p;
  if (check(env, mf_get_params(CTX(h), &p)) != MF_OK) return -1;
  return p.num_factors;
}

static void fill_params(mf_params* p, jint k, jint it, jdouble lambda, jdouble lr, jint lrm, jdouble lra, jint nb,
                        jlong seed, jboolean hs, jint mode) {
  mf_params_init(p);
  p->num_factors = k;
  p->iterations = it;
  p->lambda = lambda;
  p->learning_rate = lr;
  p->lr_method = lrm;
  p->lr_arg = lra;
  p->num_blocks = nb;
  p->seed = seed;
  p->has_seed = hs ? 1 : 0;
  p->mode = mode;
}

JNIEXPORT jlong JNICALL JFN(create)(JNIEnv* env, jclass c, jint k, jint it, jdouble lambda, jdouble lr, jint lrm,
                                    jdouble lra, jint nb, jlong seed, jboolean hs, jint mode, jdouble olr, jint oinit,
                                    jintArray devs) {
  mf_params p;
  fill_params(&p, k, it, lambda, lr, lrm, lra, nb, seed, hs, mode);
  p.online_learning_rate = olr;
  p.online_init = oinit;
  mf_ctx* ctx = NULL;
  const jsize nd = len(env, devs);
  Elems d = {0};
  if (acquire(env, &d, devs, kInt)) return 0;
  int st = mf_create(&p, (const int*)d.p, nd ? nd : 1, &ctx);
  release(env, &d, JNI_ABORT);
  return check(env, st) == MF_OK ? (jlong)(intptr_t)ctx : 0;
}

JNIEXPORT jbyteArray JNICALL JFN(commUniqueId)(JNIEnv* env, jclass c) {
  uint8_t uid[MF_UID_BYTES];
  if (check(env, mf_comm_unique_id(uid)) != MF_OK) return NULL;
  jbyteArray out = (*env)->NewByteArray(env, MF_UID_BYTES);
  if (out) (*env)->SetByteArrayRegion(env, out, 0, MF_UID_BYTES, (const jbyte*)uid);
  return out;
}

JNIEXPORT jlong JNICALL JFN(createRank)(JNIEnv* env, jclass c, jint k, jint it, jdouble lambda, jdouble lr, jint lrm,
                                        jdouble lra, jint nb, jlong seed, jboolean hs, jint mode, jint dev,
                                        jint nranks, jint rank, jbyteArray uid) {
  if (require(env, uid && len(env, uid) == MF_UID_BYTES, "uid must be the 128-byte array of commUniqueId")) return 0;
  mf_params p;
  fill_params(&p, k, it, lambda, lr, lrm, lra, nb, seed, hs, mode);
  uint8_t id[MF_UID_BYTES] = {0};
  (*env)->GetByteArrayRegion(env, uid, 0, MF_UID_BYTES, (jbyte*)id);
  mf_ctx* ctx = NULL;
  int st = mf_create_rank(&p, dev, nranks, rank, id, &ctx);
  return check(env, st) == MF_OK ? (jlong)(intptr_t)ctx : 0;
}

JNIEXPORT void JNICALL JFN(destroy)(JNIEnv* env, jclass c, jlong h) { check(env, mf_destroy(CTX(h))); }

typedef int (*ratings_fn)(mf_ctx*, const int32_t*, const int32_t*, const double*, int64_t);

/* (u, i, r) columns of one DataSet[(Int, Int, Double)]: parallel arrays of one length. */
static int rating_columns(JNIEnv* env, jintArray u, jintArray i, jdoubleArray r, jsize* n) {
  if (require(env, u && i && r, "rating columns must not be null")) return -1;
  *n = len(env, r);
  return require(env, len(env, u) == *n && len(env, i) == *n, "user, item and rating columns differ in length");
}

static void with_ratings(JNIEnv* env, jlong h, jintArray u, jintArray i, jdoubleArray r, ratings_fn fn) {
  jsize n = 0;
  if (rating_columns(env, u, i, r, &n)) return;
  Elems eu = {0}, ei = {0}, er = {0};
  if (acquire(env, &eu, u, kInt) || acquire(env, &ei, i, kInt) || acquire(env, &er, r, kDouble)) {
    release(env, &eu, JNI_ABORT);
    release(env, &ei, JNI_ABORT);
    return;
  }
  int st = fn(CTX(h), (const int32_t*)eu.p, (const int32_t*)ei.p, (const double*)er.p, n);
  release(env, &er, JNI_ABORT);
  release(env, &ei, JNI_ABORT);
  release(env, &eu, JNI_ABORT);
  check(env, st);
}

JNIEXPORT void JNICALL JFN(dsgdFit)(JNIEnv* env, jclass c, jlong h, jintArray u, jintArray i, jdoubleArray r) {
  with_ratings(env, h, u, i, r, mf_dsgd_fit);
}

JNIEXPORT void JNICALL JFN(dsgdPrepare)(JNIEnv* env, jclass c, jlong h, jintArray u, jintArray i, jdoubleArray r) {
  with_ratings(env, h, u, i, r, mf_dsgd_prepare);
}

/* ALS.train(ratings, rank, iterations, lambda) (sp/OnlineSpark.scala:125-131): mf_als_fit */
JNIEXPORT void JNICALL JFN(alsFit)(JNIEnv* env, jclass c, jlong h, jintArray u, jintArray i, jdoubleArray r,
                                   jint iterations, jdouble lambda, jint reg) {
  jsize n = 0;
  if (rating_columns(env, u, i, r, &n)) return;
  Elems eu = {0}, ei = {0}, er = {0};
  if (acquire(env, &eu, u, kInt) || acquire(env, &ei, i, kInt) || acquire(env, &er, r, kDouble)) {
    release(env, &eu, JNI_ABORT);
    release(env, &ei, JNI_ABORT);
    return;
  }
  int st = mf_als_fit(CTX(h), (const int32_t*)eu.p, (const int32_t*)ei.p, (const double*)er.p, n, iterations, lambda, reg);
  release(env, &er, JNI_ABORT);
  release(env, &ei, JNI_ABORT);
  release(env, &eu, JNI_ABORT);
  check(env, st);
}

/* ALS.trainImplicit(ratings, rank, iterations, lambda, alpha): mf_als_fit_implicit */
JNIEXPORT void JNICALL JFN(alsFitImplicit)(JNIEnv* env, jclass c, jlong h, jintArray u, jintArray i, jdoubleArray r,
                                           jint iterations, jdouble lambda, jint reg, jdouble alpha) {
  jsize n = 0;
  if (rating_columns(env, u, i, r, &n)) return;
  Elems eu = {0}, ei = {0}, er = {0};
  if (acquire(env, &eu, u, kInt) || acquire(env, &ei, i, kInt) || acquire(env, &er, r, kDouble)) {
    release(env, &eu, JNI_ABORT);
    release(env, &ei, JNI_ABORT);
    return;
  }
  int st = mf_als_fit_implicit(CTX(h), (const int32_t*)eu.p, (const int32_t*)ei.p, (const double*)er.p, n, iterations,
                               lambda, reg, alpha);
  release(env, &er, JNI_ABORT);
  release(env, &ei, JNI_ABORT);
  release(env, &eu, JNI_ABORT);
  check(env, st);
}

/* The conjugate-gradient half-sweeps: alsPrepare (mf_als_prepare) once, then run calls of any kind; the fit
   calls are prepare + 2 * iterations half-sweeps.  alpha < 0 in als_cg_call: the explicit calls. */
static void als_cg_call(JNIEnv* env, jlong h, jintArray u, jintArray i, jdoubleArray r, int fit, jint iterations,
                        jdouble lambda, jint reg, jdouble alpha, jint cgSteps) {
  jsize n = 0;
  if (rating_columns(env, u, i, r, &n)) return;
  Elems eu = {0}, ei = {0}, er = {0};
  if (acquire(env, &eu, u, kInt) || acquire(env, &ei, i, kInt) || acquire(env, &er, r, kDouble)) {
    release(env, &eu, JNI_ABORT);
    release(env, &ei, JNI_ABORT);
    return;
  }
  const int32_t* pu = (const int32_t*)eu.p;
  const int32_t* pi = (const int32_t*)ei.p;
  const double* pr = (const double*)er.p;
  int st;
  if (!fit) st = mf_als_prepare(CTX(h), pu, pi, pr, n);
  else if (alpha < 0) st = mf_als_fit_cg(CTX(h), pu, pi, pr, n, iterations, lambda, reg, cgSteps);
  else st = mf_als_fit_implicit_cg(CTX(h), pu, pi, pr, n, iterations, lambda, reg, alpha, cgSteps);
  release(env, &er, JNI_ABORT);
  release(env, &ei, JNI_ABORT);
  release(env, &eu, JNI_ABORT);
  check(env, st);
}

JNIEXPORT void JNICALL JFN(alsPrepare)(JNIEnv* env, jclass c, jlong h, jintArray u, jintArray i, jdoubleArray r) {
  als_cg_call(env, h, u, i, r, 0, 0, 0.0, 0, -1.0, 0);
}

JNIEXPORT void JNICALL JFN(alsFitCg)(JNIEnv* env, jclass c, jlong h, jintArray u, jintArray i, jdoubleArray r,
                                     jint iterations, jdouble lambda, jint reg, jint cgSteps) {
  als_cg_call(env, h, u, i, r, 1, iterations, lambda, reg, -1.0, cgSteps);
}

JNIEXPORT void JNICALL JFN(alsFitImplicitCg)(JNIEnv* env, jclass c, jlong h, jintArray u, jintArray i, jdoubleArray r,
                                             jint iterations, jdouble lambda, jint reg, jdouble alpha, jint cgSteps) {
  if (alpha < 0) {  /* (the helper reads a negative alpha as "explicit") */
    check(env, mf_als_run_implicit_cg(CTX(h), 0, lambda, reg, alpha, cgSteps));
    return;
  }
  als_cg_call(env, h, u, i, r, 1, iterations, lambda, reg, alpha, cgSteps);
}

JNIEXPORT void JNICALL JFN(alsRunCg)(JNIEnv* env, jclass c, jlong h, jlong halfSweeps, jdouble lambda, jint reg,
                                     jint cgSteps) {
  check(env, mf_als_run_cg(CTX(h), halfSweeps, lambda, reg, cgSteps));
}

JNIEXPORT void JNICALL JFN(alsRunImplicitCg)(JNIEnv* env, jclass c, jlong h, jlong halfSweeps, jdouble lambda, jint reg,
                                             jdouble alpha, jint cgSteps) {
  check(env, mf_als_run_implicit_cg(CTX(h), halfSweeps, lambda, reg, alpha, cgSteps));
}

/* The non-negative half-sweeps (MLlib's nonnegative = true): mf_als_fit_nonneg, or with alpha >= 0
   mf_als_fit_implicit_nonneg. */
static void als_nonneg_fit(JNIEnv* env, jlong h, jintArray u, jintArray i, jdoubleArray r, jint iterations,
                           jdouble lambda, jint reg, int implicit, jdouble alpha) {
  jsize n = 0;
  if (rating_columns(env, u, i, r, &n)) return;
  Elems eu = {0}, ei = {0}, er = {0};
  if (acquire(env, &eu, u, kInt) || acquire(env, &ei, i, kInt) || acquire(env, &er, r, kDouble)) {
    release(env, &eu, JNI_ABORT);
    release(env, &ei, JNI_ABORT);
    return;
  }
  const int32_t* pu = (const int32_t*)eu.p;
  const int32_t* pi = (const int32_t*)ei.p;
  const double* pr = (const double*)er.p;
  int st;
  if (implicit) st = mf_als_fit_implicit_nonneg(CTX(h), pu, pi, pr, n, iterations, lambda, reg, alpha);
  else st = mf_als_fit_nonneg(CTX(h), pu, pi, pr, n, iterations, lambda, reg);
  release(env, &er, JNI_ABORT);
  release(env, &ei, JNI_ABORT);
  release(env, &eu, JNI_ABORT);
  check(env, st);
}

JNIEXPORT void JNICALL JFN(alsFitNonneg)(JNIEnv* env, jclass c, jlong h, jintArray u, jintArray i, jdoubleArray r,
                                         jint iterations, jdouble lambda, jint reg) {
  als_nonneg_fit(env, h, u, i, r, iterations, lambda, reg, 0, 0.0);
}

JNIEXPORT void JNICALL JFN(alsFitImplicitNonneg)(JNIEnv* env, jclass c, jlong h, jintArray u, jintArray i,
                                                 jdoubleArray r, jint iterations, jdouble lambda, jint reg,
                                                 jdouble alpha) {
  als_nonneg_fit(env, h, u, i, r, iterations, lambda, reg, 1, alpha);
}

JNIEXPORT void JNICALL JFN(alsRunNonneg)(JNIEnv* env, jclass c, jlong h, jlong halfSweeps, jdouble lambda, jint reg) {
  check(env, mf_als_run_nonneg(CTX(h), halfSweeps, lambda, reg));
}

JNIEXPORT void JNICALL JFN(alsRunImplicitNonneg)(JNIEnv* env, jclass c, jlong h, jlong halfSweeps, jdouble lambda,
                                                 jint reg, jdouble alpha) {
  check(env, mf_als_run_implicit_nonneg(CTX(h), halfSweeps, lambda, reg, alpha));
}

/* Incremental ALS: mf_als_append, mf_als_run_rows, mf_als_update (users first, then items). */
static mf_als_solve als_how(jdouble lambda, jint reg, jint implicit, jdouble alpha, jint solver, jint cgSteps) {
  mf_als_solve how = {0};
  how.lambda = lambda;
  how.reg = reg;
  how.implicit = implicit;
  how.alpha = alpha;
  how.solver = solver;
  how.cg_steps = cgSteps;
  return how;
}

JNIEXPORT void JNICALL JFN(alsAppend)(JNIEnv* env, jclass c, jlong h, jintArray u, jintArray i, jdoubleArray r) {
  with_ratings(env, h, u, i, r, mf_als_append);
}

JNIEXPORT jlong JNICALL JFN(alsRunRows)(JNIEnv* env, jclass c, jlong h, jint side, jintArray ids, jdouble lambda,
                                        jint reg, jint implicit, jdouble alpha, jint solver, jint cgSteps) {
  if (require(env, ids != NULL, "ids must not be null")) return 0;
  const mf_als_solve how = als_how(lambda, reg, implicit, alpha, solver, cgSteps);
  Elems e = {0};
  if (acquire(env, &e, ids, kInt)) return 0;
  int64_t solved = 0;
  int st = mf_als_run_rows(CTX(h), side, (const int32_t*)e.p, len(env, ids), &how, &solved);
  release(env, &e, JNI_ABORT);
  check(env, st);
  return (jlong)solved;
}

JNIEXPORT void JNICALL JFN(alsUpdate)(JNIEnv* env, jclass c, jlong h, jintArray u, jintArray i, jdoubleArray r,
                                      jdouble lambda, jint reg, jint implicit, jdouble alpha, jint solver,
                                      jint cgSteps, jint rounds, jintArray solvedOut) {
  jsize n = 0;
  if (rating_columns(env, u, i, r, &n)) return;
  if (require(env, !solvedOut || len(env, solvedOut) >= 2, "solvedOut must hold 2 entries")) return;
  const mf_als_solve how = als_how(lambda, reg, implicit, alpha, solver, cgSteps);
  Elems eu = {0}, ei = {0}, er = {0};
  if (acquire(env, &eu, u, kInt) || acquire(env, &ei, i, kInt) || acquire(env, &er, r, kDouble)) {
    release(env, &eu, JNI_ABORT);
    release(env, &ei, JNI_ABORT);
    return;
  }
  int64_t su = 0, si = 0;
  int st = mf_als_update(CTX(h), (const int32_t*)eu.p, (const int32_t*)ei.p, (const double*)er.p, n, &how, rounds,
                         &su, &si);
  release(env, &er, JNI_ABORT);
  release(env, &ei, JNI_ABORT);
  release(env, &eu, JNI_ABORT);
  if (check(env, st) != MF_OK || !solvedOut) return;
  Elems eo = {0};
  if (acquire(env, &eo, solvedOut, kInt)) return;
  ((jint*)eo.p)[0] = (jint)su;
  ((jint*)eo.p)[1] = (jint)si;
  release(env, &eo, 0);
}

/* mf_als_objective: lossOut (length >= 8) receives total, fit, unobserved, reg_user, reg_item, ratings,
   user_rows, item_rows; the return value is total.  mf_als_run_until: historyOut (may be null, length >=
   maxIterations + 1) receives the objective on entry and after every iteration; returns the iterations taken. */
JNIEXPORT jdouble JNICALL JFN(alsObjective)(JNIEnv* env, jclass c, jlong h, jdouble lambda, jint reg, jint implicit,
                                            jdouble alpha, jdoubleArray lossOut) {
  if (require(env, !lossOut || len(env, lossOut) >= 8, "lossOut must hold 8 entries")) return 0.0;
  const mf_als_solve how = als_how(lambda, reg, implicit, alpha, MF_ALS_SOLVER_CHOLESKY, 0);
  mf_als_loss loss;
  if (check(env, mf_als_objective(CTX(h), &how, &loss)) != MF_OK) return 0.0;
  if (lossOut) {
    Elems eo = {0};
    if (acquire(env, &eo, lossOut, kDouble)) return 0.0;
    double* o = (double*)eo.p;
    o[0] = loss.total;
    o[1] = loss.fit;
    o[2] = loss.unobserved;
    o[3] = loss.reg_user;
    o[4] = loss.reg_item;
    o[5] = (double)loss.ratings;
    o[6] = (double)loss.user_rows;
    o[7] = (double)loss.item_rows;
    release(env, &eo, 0);
  }
  return loss.total;
}

JNIEXPORT jint JNICALL JFN(alsRunUntil)(JNIEnv* env, jclass c, jlong h, jdouble lambda, jint reg, jint implicit,
                                        jdouble alpha, jint solver, jint cgSteps, jint maxIterations, jdouble relTol,
                                        jdoubleArray historyOut) {
  if (require(env, maxIterations >= 0, "maxIterations must be >= 0")) return 0;
  if (require(env, !historyOut || (jlong)len(env, historyOut) >= (jlong)maxIterations + 1,
              "historyOut must hold maxIterations + 1 entries"))
    return 0;
  const mf_als_solve how = als_how(lambda, reg, implicit, alpha, solver, cgSteps);
  Elems eh = {0};
  if (historyOut && acquire(env, &eh, historyOut, kDouble)) return 0;
  int32_t t = 0;
  int st = mf_als_run_until(CTX(h), &how, maxIterations, relTol, &t, historyOut ? (double*)eh.p : NULL);
  if (historyOut) release(env, &eh, 0);
  check(env, st);
  return (jint)t;
}

/* Removal: mf_als_remove, mf_als_remove_rows, mf_als_retract.  foundOut (may be null, length >= n) receives
   0 / 1 per entry; the return value is the number of ratings removed. */
static int acquire_all(JNIEnv* env, Elems* e, const jarray* a, const int* kind, int n);
static jlong als_remove_or_retract(JNIEnv* env, jlong h, jintArray u, jintArray i, const mf_als_solve* how, jint rounds,
                                   jbyteArray foundOut, jintArray solvedOut) {
  if (require(env, u && i && len(env, u) == len(env, i), "users and items must match in length")) return 0;
  const jsize n = len(env, u);
  if (require(env, !foundOut || len(env, foundOut) >= n, "foundOut must hold an entry per pair")) return 0;
  if (require(env, !solvedOut || len(env, solvedOut) >= 2, "solvedOut must hold 2 entries")) return 0;
  uint8_t* found = foundOut && n ? (uint8_t*)malloc((size_t)n) : NULL;
  if (require(env, !(foundOut && n) || found, "out of memory")) return 0;
  Elems e[2];
  const jarray arr[2] = {u, i};
  const int kind[2] = {kInt, kInt};
  if (acquire_all(env, e, arr, kind, 2)) {
    free(found);
    return 0;
  }
  const int32_t* pu = n ? (const int32_t*)e[0].p : NULL;
  const int32_t* pi = n ? (const int32_t*)e[1].p : NULL;
  int64_t removed = 0, su = 0, si = 0;
  int st = how ? mf_als_retract(CTX(h), pu, pi, n, how, rounds, found, &removed, &su, &si)
               : mf_als_remove(CTX(h), pu, pi, n, found, &removed);
  for (int x = 1; x >= 0; --x) release(env, &e[x], JNI_ABORT);
  if (check(env, st) == MF_OK) {
    Elems eo = {0};
    if (found) (*env)->SetByteArrayRegion(env, foundOut, 0, n, (const jbyte*)found);
    if (solvedOut && !acquire(env, &eo, solvedOut, kInt)) {
      ((jint*)eo.p)[0] = (jint)su;
      ((jint*)eo.p)[1] = (jint)si;
      release(env, &eo, 0);
    }
  }
  free(found);
  return (jlong)removed;
}

JNIEXPORT jlong JNICALL JFN(alsRemove)(JNIEnv* env, jclass c, jlong h, jintArray u, jintArray i, jbyteArray foundOut) {
  return als_remove_or_retract(env, h, u, i, NULL, 0, foundOut, NULL);
}

JNIEXPORT jlong JNICALL JFN(alsRemoveRows)(JNIEnv* env, jclass c, jlong h, jint side, jintArray ids) {
  if (require(env, ids != NULL, "ids must not be null")) return 0;
  Elems e = {0};
  if (acquire(env, &e, ids, kInt)) return 0;
  int64_t removed = 0;
  int st = mf_als_remove_rows(CTX(h), side, (const int32_t*)e.p, len(env, ids), &removed);
  release(env, &e, JNI_ABORT);
  check(env, st);
  return (jlong)removed;
}

JNIEXPORT jlong JNICALL JFN(alsRetract)(JNIEnv* env, jclass c, jlong h, jintArray u, jintArray i, jdouble lambda,
                                        jint reg, jint implicit, jdouble alpha, jint solver, jint cgSteps, jint rounds,
                                        jbyteArray foundOut, jintArray solvedOut) {
  const mf_als_solve how = als_how(lambda, reg, implicit, alpha, solver, cgSteps);
  return als_remove_or_retract(env, h, u, i, &how, rounds, foundOut, solvedOut);
}

JNIEXPORT void JNICALL JFN(dsgdRun)(JNIEnv* env, jclass c, jlong h, jlong supersteps) {
  check(env, mf_dsgd_run(CTX(h), supersteps));
}

JNIEXPORT void JNICALL JFN(dsgdRestart)(JNIEnv* env, jclass c, jlong h) { check(env, mf_dsgd_restart(CTX(h))); }

JNIEXPORT void JNICALL JFN(sync)(JNIEnv* env, jclass c, jlong h) { check(env, mf_sync(CTX(h))); }

JNIEXPORT jlong JNICALL JFN(numFactors)(JNIEnv* env, jclass c, jlong h, jint side) {
  int64_t n = 0;
  check(env, mf_num_factors(CTX(h), side, &n));
  return n;
}

JNIEXPORT jlong JNICALL JFN(getFactors)(JNIEnv* env, jclass c, jlong h, jint side, jintArray ids, jdoubleArray vecs) {
  const jlong k = rank_of(env, h);
  if (k < 0) return 0;
  const jsize cap = len(env, ids);
  if (require(env, ids && vecs && (jlong)len(env, vecs) >= (jlong)cap * k, "vecs must hold ids.length * k doubles"))
    return 0;
  int64_t w = 0;
  Elems ei = {0}, ev = {0};
  if (acquire(env, &ei, ids, kInt) || acquire(env, &ev, vecs, kDouble)) {
    release(env, &ei, JNI_ABORT);
    return 0;
  }
  int st = mf_get_factors(CTX(h), side, (int32_t*)ei.p, (double*)ev.p, cap, &w);
  release(env, &ev, st == MF_OK ? 0 : JNI_ABORT);
  release(env, &ei, st == MF_OK ? 0 : JNI_ABORT);
  check(env, st);
  return w;
}

JNIEXPORT void JNICALL JFN(setFactors)(JNIEnv* env, jclass c, jlong h, jint side, jintArray ids, jdoubleArray vecs) {
  const jlong k = rank_of(env, h);
  if (k < 0) return;
  const jsize n = len(env, ids);
  if (require(env, ids && vecs && (jlong)len(env, vecs) >= (jlong)n * k, "vecs must hold ids.length * k doubles"))
    return;
  Elems ei = {0}, ev = {0};
  if (acquire(env, &ei, ids, kInt) || acquire(env, &ev, vecs, kDouble)) {
    release(env, &ei, JNI_ABORT);
    return;
  }
  int st = mf_set_factors(CTX(h), side, (const int32_t*)ei.p, (const double*)ev.p, n);
  release(env, &ev, JNI_ABORT);
  release(env, &ei, JNI_ABORT);
  check(env, st);
}

JNIEXPORT void JNICALL JFN(predict)(JNIEnv* env, jclass c, jlong h, jintArray u, jintArray i, jdoubleArray out,
                                    jbyteArray found) {
  if (require(env, u && i && out && found, "arguments must not be null")) return;
  const jsize n = len(env, u);
  if (require(env, len(env, i) == n && len(env, out) >= n && len(env, found) >= n,
              "items must match users in length; out and found must hold users.length entries"))
    return;
  Elems eu = {0}, ei = {0}, eo = {0}, ef = {0};
  if (acquire(env, &eu, u, kInt) || acquire(env, &ei, i, kInt) || acquire(env, &eo, out, kDouble) ||
      acquire(env, &ef, found, kByte)) {
    release(env, &eo, JNI_ABORT);
    release(env, &ei, JNI_ABORT);
    release(env, &eu, JNI_ABORT);
    return;
  }
  int st = mf_predict(CTX(h), (const int32_t*)eu.p, (const int32_t*)ei.p, n, (double*)eo.p, (uint8_t*)ef.p);
  release(env, &ef, st == MF_OK ? 0 : JNI_ABORT);
  release(env, &eo, st == MF_OK ? 0 : JNI_ABORT);
  release(env, &ei, JNI_ABORT);
  release(env, &eu, JNI_ABORT);
  check(env, st);
}

JNIEXPORT void JNICALL JFN(recommend)(JNIEnv* env, jclass c, jlong h, jint side, jintArray q, jint top, jintArray xq,
                                      jintArray xc, jintArray ids, jdoubleArray scores, jintArray counts) {
  if (require(env, q && ids && counts, "queries, idsOut and countsOut must not be null")) return;
  if (require(env, top >= 1 && top <= MF_RECOMMEND_MAX_TOP, "topN out of range")) return;
  const jsize n = len(env, q);
  if (require(env, (jlong)len(env, ids) >= (jlong)n * top && (!scores || (jlong)len(env, scores) >= (jlong)n * top) &&
                       len(env, counts) >= n,
              "idsOut / scoresOut must hold queries.length * topN entries and countsOut queries.length"))
    return;
  if (require(env, (!xq && !xc) || (xq && xc && len(env, xq) == len(env, xc)),
              "exclQuery and exclCand must both be null or match in length"))
    return;
  const jsize ne = xq ? len(env, xq) : 0;
  Elems eq = {0}, exq = {0}, exc = {0}, ei = {0}, es = {0}, ec = {0};
  if (acquire(env, &eq, q, kInt) || acquire(env, &exq, xq, kInt) || acquire(env, &exc, xc, kInt) ||
      acquire(env, &ei, ids, kInt) || acquire(env, &es, scores, kDouble) || acquire(env, &ec, counts, kInt)) {
    release(env, &es, JNI_ABORT);
    release(env, &ei, JNI_ABORT);
    release(env, &exc, JNI_ABORT);
    release(env, &exq, JNI_ABORT);
    release(env, &eq, JNI_ABORT);
    return;
  }
  int st = mf_recommend(CTX(h), side, (const int32_t*)eq.p, n, top, ne ? (const int32_t*)exq.p : NULL,
                        ne ? (const int32_t*)exc.p : NULL, ne, (int32_t*)ei.p, (double*)es.p, (int32_t*)ec.p);
  release(env, &ec, st == MF_OK ? 0 : JNI_ABORT);
  release(env, &es, st == MF_OK ? 0 : JNI_ABORT);
  release(env, &ei, st == MF_OK ? 0 : JNI_ABORT);
  release(env, &exc, JNI_ABORT);
  release(env, &exq, JNI_ABORT);
  release(env, &eq, JNI_ABORT);
  check(env, st);
}

JNIEXPORT void JNICALL JFN(rankEval)(JNIEnv* env, jclass c, jlong h, jint side, jintArray gq, jintArray gc, jint top,
                                     jintArray xq, jintArray xc, jdoubleArray metrics) {
  if (require(env, gq && gc && len(env, gq) == len(env, gc), "gtQuery and gtCand must match in length")) return;
  if (require(env, metrics && len(env, metrics) >= 8, "metricsOut must hold 8 entries")) return;
  if (require(env, top >= 1 && top <= MF_RECOMMEND_MAX_TOP, "topN out of range")) return;
  if (require(env, (!xq && !xc) || (xq && xc && len(env, xq) == len(env, xc)),
              "exclQuery and exclCand must both be null or match in length"))
    return;
  const jsize ng = len(env, gq), ne = xq ? len(env, xq) : 0;
  Elems eq = {0}, ec = {0}, exq = {0}, exc = {0}, em = {0};
  if (acquire(env, &eq, gq, kInt) || acquire(env, &ec, gc, kInt) || acquire(env, &exq, xq, kInt) ||
      acquire(env, &exc, xc, kInt) || acquire(env, &em, metrics, kDouble)) {
    release(env, &exc, JNI_ABORT);
    release(env, &exq, JNI_ABORT);
    release(env, &ec, JNI_ABORT);
    release(env, &eq, JNI_ABORT);
    return;
  }
  mf_rank_metrics m;
  int st = mf_rank_eval(CTX(h), side, ng ? (const int32_t*)eq.p : NULL, ng ? (const int32_t*)ec.p : NULL, ng, top,
                        ne ? (const int32_t*)exq.p : NULL, ne ? (const int32_t*)exc.p : NULL, ne, &m, NULL, NULL, NULL,
                        0);
  if (st == MF_OK) {
    double* o = (double*)em.p;
    o[0] = (double)m.queries;
    o[1] = (double)m.hits;
    o[2] = m.precision;
    o[3] = m.recall;
    o[4] = m.map;
    o[5] = m.ndcg;
    o[6] = m.mrr;
    o[7] = m.hit_rate;
  }
  release(env, &em, st == MF_OK ? 0 : JNI_ABORT);
  release(env, &exc, JNI_ABORT);
  release(env, &exq, JNI_ABORT);
  release(env, &ec, JNI_ABORT);
  release(env, &eq, JNI_ABORT);
  check(env, st);
}

/* Elements of up to 8 arrays, acquired in order; on failure the ones already held are discarded. */
static int acquire_all(JNIEnv* env, Elems* e, const jarray* a, const int* kind, int n) {
  for (int x = 0; x < n; ++x) {
    if (acquire(env, &e[x], a[x], kind[x])) {
      while (x-- > 0) release(env, &e[x], JNI_ABORT);
      return -1;
    }
  }
  return 0;
}

JNIEXPORT void JNICALL JFN(pairRanks)(JNIEnv* env, jclass c, jlong h, jint side, jintArray q, jintArray cd,
                                      jintArray xq, jintArray xc, jintArray ranks, jintArray valid,
                                      jdoubleArray scores) {
  if (require(env, q && cd && len(env, q) == len(env, cd), "queries and cands must match in length")) return;
  const jsize n = len(env, q), ne = xq ? len(env, xq) : 0;
  if (require(env, ranks && len(env, ranks) >= n, "ranksOut must hold one entry per pair")) return;
  if (require(env, (!valid || len(env, valid) >= n) && (!scores || len(env, scores) >= n),
              "validOut / scoresOut must be null or hold one entry per pair"))
    return;
  if (require(env, (!xq && !xc) || (xq && xc && len(env, xq) == len(env, xc)),
              "exclQuery and exclCand must both be null or match in length"))
    return;
  Elems e[7];
  const jarray arr[7] = {q, cd, xq, xc, ranks, valid, scores};
  const int kind[7] = {kInt, kInt, kInt, kInt, kInt, kInt, kDouble};
  if (acquire_all(env, e, arr, kind, 7)) return;
  int st = mf_pair_ranks(CTX(h), side, n ? (const int32_t*)e[0].p : NULL, n ? (const int32_t*)e[1].p : NULL, n,
                         ne ? (const int32_t*)e[2].p : NULL, ne ? (const int32_t*)e[3].p : NULL, ne, (int32_t*)e[4].p,
                         (int32_t*)e[5].p, (double*)e[6].p);
  for (int x = 6; x >= 4; --x) release(env, &e[x], st == MF_OK ? 0 : JNI_ABORT);
  for (int x = 3; x >= 0; --x) release(env, &e[x], JNI_ABORT);
  check(env, st);
}

JNIEXPORT void JNICALL JFN(onlinePrequential)(JNIEnv* env, jclass c, jlong h, jintArray u, jintArray i, jdoubleArray r,
                                              jint flavour, jint parts, jint top, jintArray xu, jintArray xi,
                                              jdoubleArray metrics, jintArray ranks) {
  if (require(env, u && i && r && len(env, u) == len(env, i) && len(env, u) == len(env, r),
              "users, items and ratings must match in length"))
    return;
  const jsize n = len(env, u), ne = xu ? len(env, xu) : 0;
  if (require(env, metrics && len(env, metrics) >= 12, "metricsOut must hold 12 entries")) return;
  if (require(env, !ranks || len(env, ranks) >= n, "ranksOut must be null or hold one entry per event")) return;
  if (require(env, (!xu && !xi) || (xu && xi && len(env, xu) == len(env, xi)),
              "exclUser and exclItem must both be null or match in length"))
    return;
  Elems e[7];
  const jarray arr[7] = {u, i, r, xu, xi, metrics, ranks};
  const int kind[7] = {kInt, kInt, kDouble, kInt, kInt, kDouble, kInt};
  if (acquire_all(env, e, arr, kind, 7)) return;
  mf_prequential m;
  int st = mf_online_prequential(CTX(h), n ? (const int32_t*)e[0].p : NULL, n ? (const int32_t*)e[1].p : NULL,
                                 n ? (const double*)e[2].p : NULL, n, flavour, parts, top,
                                 ne ? (const int32_t*)e[3].p : NULL, ne ? (const int32_t*)e[4].p : NULL, ne, &m,
                                 (int32_t*)e[6].p, NULL, NULL);
  if (st == MF_OK) {
    double* o = (double*)e[5].p;
    o[0] = (double)m.events;
    o[1] = (double)m.evaluated;
    o[2] = (double)m.cold;
    o[3] = (double)m.excluded;
    o[4] = (double)m.hits;
    o[5] = m.sum_ndcg;
    o[6] = m.sum_rr;
    o[7] = m.sum_pr;
    o[8] = m.ndcg;
    o[9] = m.mrr;
    o[10] = m.hit_rate;
    o[11] = m.mpr;
  }
  for (int x = 6; x >= 5; --x) release(env, &e[x], st == MF_OK ? 0 : JNI_ABORT);
  for (int x = 4; x >= 0; --x) release(env, &e[x], JNI_ABORT);
  check(env, st);
}

// metricsOut[0 .. 11] of the prequential natives from the record
static void store_prequential(double* o, const mf_prequential* m) {
  o[0] = (double)m->events;
  o[1] = (double)m->evaluated;
  o[2] = (double)m->cold;
  o[3] = (double)m->excluded;
  o[4] = (double)m->hits;
  o[5] = m->sum_ndcg;
  o[6] = m->sum_rr;
  o[7] = m->sum_pr;
  o[8] = m->ndcg;
  o[9] = m->mrr;
  o[10] = m->hit_rate;
  o[11] = m->mpr;
}

// the negatives' count against MF_NEG_MAX and the length of sampledOut (may be null)
static int sampled_shape(JNIEnv* env, jsize n, jint negatives, jintArray sampled) {
  if (require(env, negatives >= 0 && negatives <= MF_NEG_MAX, "negatives must be in 0 .. 64")) return 1;
  return require(env, !sampled || (jlong)len(env, sampled) >= (jlong)n * negatives,
                 "sampledOut must be null or hold users.length * negatives entries");
}

JNIEXPORT void JNICALL JFN(onlineUpdateSampled)(JNIEnv* env, jclass c, jlong h, jintArray u, jintArray i,
                                                jdoubleArray r, jint flavour, jint negatives, jdouble negRating,
                                                jlong seed, jlong firstEvent, jintArray sampled) {
  jsize n = 0;
  if (rating_columns(env, u, i, r, &n)) return;
  if (sampled_shape(env, n, negatives, sampled)) return;
  Elems e[4];
  const jarray arr[4] = {u, i, r, sampled};
  const int kind[4] = {kInt, kInt, kDouble, kInt};
  if (acquire_all(env, e, arr, kind, 4)) return;
  int st = mf_online_update_sampled(CTX(h), (const int32_t*)e[0].p, (const int32_t*)e[1].p, (const double*)e[2].p, n,
                                    flavour, negatives, negRating, seed, firstEvent, (int32_t*)e[3].p, NULL, NULL);
  release(env, &e[3], st == MF_OK ? 0 : JNI_ABORT);
  for (int x = 2; x >= 0; --x) release(env, &e[x], JNI_ABORT);
  check(env, st);
}

JNIEXPORT void JNICALL JFN(onlinePrequentialSampled)(JNIEnv* env, jclass c, jlong h, jintArray u, jintArray i,
                                                     jdoubleArray r, jint flavour, jint top, jintArray xu,
                                                     jintArray xi, jdoubleArray metrics, jintArray ranks,
                                                     jint negatives, jdouble negRating, jlong seed, jlong firstEvent,
                                                     jintArray sampled) {
  if (require(env, u && i && r && len(env, u) == len(env, i) && len(env, u) == len(env, r),
              "users, items and ratings must match in length"))
    return;
  const jsize n = len(env, u), ne = xu ? len(env, xu) : 0;
  if (require(env, metrics && len(env, metrics) >= 12, "metricsOut must hold 12 entries")) return;
  if (require(env, !ranks || len(env, ranks) >= n, "ranksOut must be null or hold one entry per event")) return;
  if (require(env, (!xu && !xi) || (xu && xi && len(env, xu) == len(env, xi)),
              "exclUser and exclItem must both be null or match in length"))
    return;
  if (sampled_shape(env, n, negatives, sampled)) return;
  Elems e[8];
  const jarray arr[8] = {u, i, r, xu, xi, metrics, ranks, sampled};
  const int kind[8] = {kInt, kInt, kDouble, kInt, kInt, kDouble, kInt, kInt};
  if (acquire_all(env, e, arr, kind, 8)) return;
  mf_prequential m;
  int st = mf_online_prequential_sampled(CTX(h), n ? (const int32_t*)e[0].p : NULL, n ? (const int32_t*)e[1].p : NULL,
                                         n ? (const double*)e[2].p : NULL, n, flavour, top,
                                         ne ? (const int32_t*)e[3].p : NULL, ne ? (const int32_t*)e[4].p : NULL, ne, &m,
                                         (int32_t*)e[6].p, NULL, NULL, negatives, negRating, seed, firstEvent,
                                         (int32_t*)e[7].p);
  if (st == MF_OK) store_prequential((double*)e[5].p, &m);
  for (int x = 7; x >= 5; --x) release(env, &e[x], st == MF_OK ? 0 : JNI_ABORT);
  for (int x = 4; x >= 0; --x) release(env, &e[x], JNI_ABORT);
  check(env, st);
}

/* ---- the resident seen set (mf_seen_*) and the four readers that take it ---- */
static jlong seen_put(JNIEnv* env, jlong h, jintArray u, jintArray i, int add) {
  if (require(env, u && i && len(env, u) == len(env, i), "users and items must match in length")) return 0;
  const jsize n = len(env, u);
  Elems e[2];
  const jarray arr[2] = {u, i};
  const int kind[2] = {kInt, kInt};
  if (acquire_all(env, e, arr, kind, 2)) return 0;
  int64_t ignored = 0;
  const int32_t* pu = n ? (const int32_t*)e[0].p : NULL;
  const int32_t* pi = n ? (const int32_t*)e[1].p : NULL;
  int st = add ? mf_seen_add(CTX(h), pu, pi, n, &ignored) : mf_seen_set(CTX(h), pu, pi, n, &ignored);
  for (int x = 1; x >= 0; --x) release(env, &e[x], JNI_ABORT);
  check(env, st);
  return (jlong)ignored;
}

JNIEXPORT jlong JNICALL JFN(seenSet)(JNIEnv* env, jclass c, jlong h, jintArray u, jintArray i) {
  return seen_put(env, h, u, i, 0);
}

JNIEXPORT jlong JNICALL JFN(seenAdd)(JNIEnv* env, jclass c, jlong h, jintArray u, jintArray i) {
  return seen_put(env, h, u, i, 1);
}

/* mf_seen_remove: returns the distinct held pairs removed; ignoredOut (may be null, length >= 1) the pairs
   naming an unknown id. */
JNIEXPORT jlong JNICALL JFN(seenRemove)(JNIEnv* env, jclass c, jlong h, jintArray u, jintArray i, jintArray ignoredOut) {
  if (require(env, u && i && len(env, u) == len(env, i), "users and items must match in length")) return 0;
  if (require(env, !ignoredOut || len(env, ignoredOut) >= 1, "ignoredOut must hold 1 entry")) return 0;
  const jsize n = len(env, u);
  Elems e[2];
  const jarray arr[2] = {u, i};
  const int kind[2] = {kInt, kInt};
  if (acquire_all(env, e, arr, kind, 2)) return 0;
  int64_t removed = 0, ignored = 0;
  int st = mf_seen_remove(CTX(h), n ? (const int32_t*)e[0].p : NULL, n ? (const int32_t*)e[1].p : NULL, n, &removed,
                          &ignored);
  for (int x = 1; x >= 0; --x) release(env, &e[x], JNI_ABORT);
  Elems eo = {0};
  if (check(env, st) == MF_OK && ignoredOut && !acquire(env, &eo, ignoredOut, kInt)) {
    ((jint*)eo.p)[0] = (jint)ignored; /* at most n < 2^31 */
    release(env, &eo, 0);
  }
  return (jlong)removed;
}

JNIEXPORT void JNICALL JFN(seenFromAls)(JNIEnv* env, jclass c, jlong h) { check(env, mf_seen_from_als(CTX(h))); }

JNIEXPORT void JNICALL JFN(seenClear)(JNIEnv* env, jclass c, jlong h) { check(env, mf_seen_clear(CTX(h))); }

JNIEXPORT jlong JNICALL JFN(seenCount)(JNIEnv* env, jclass c, jlong h) {
  int64_t pairs = 0;
  check(env, mf_seen_count(CTX(h), &pairs));
  return (jlong)pairs;
}

/* ---- BPR training on the seen set (mf_bpr_run, mf_bpr_step_triples, mf_bpr_fit) ----
   statsOut (may be null, length >= 4): slots, void slots, user rows written, item rows written (exact in a
   double below 2^53). */
static mf_bpr_params bpr_params_of(jdouble lr, jdouble lambda, jint batch, jint scale, jint redraws, jlong seed) {
  mf_bpr_params p = {0};
  p.lr = lr;
  p.lambda = lambda;
  p.batch = batch;
  p.scale = scale;
  p.redraws = redraws;
  p.seed = seed;
  return p;
}

static void bpr_finish(JNIEnv* env, int st, const mf_bpr_stats* s, jdoubleArray statsOut) {
  if (st == MF_OK && statsOut) {
    Elems eo;
    if (acquire(env, &eo, statsOut, kDouble)) return;
    double* o = (double*)eo.p;
    o[0] = (double)s->slots;
    o[1] = (double)s->void_slots;
    o[2] = (double)s->user_rows_written;
    o[3] = (double)s->item_rows_written;
    release(env, &eo, 0);
  }
  check(env, st);
}

JNIEXPORT void JNICALL JFN(bprRun)(JNIEnv* env, jclass c, jlong h, jdouble lr, jdouble lambda, jint batch, jint scale,
                                   jint redraws, jlong seed, jlong firstStep, jlong steps, jdoubleArray statsOut) {
  if (require(env, !statsOut || len(env, statsOut) >= 4, "statsOut must hold 4 entries")) return;
  const mf_bpr_params p = bpr_params_of(lr, lambda, batch, scale, redraws, seed);
  mf_bpr_stats s = {0, 0, 0, 0};
  bpr_finish(env, mf_bpr_run(CTX(h), &p, firstStep, steps, &s), &s, statsOut);
}

JNIEXPORT void JNICALL JFN(bprStepTriples)(JNIEnv* env, jclass c, jlong h, jdouble lr, jdouble lambda, jint scale,
                                           jintArray u, jintArray pos, jintArray neg, jdoubleArray statsOut) {
  if (require(env, u && pos && neg && len(env, u) == len(env, pos) && len(env, u) == len(env, neg),
              "users, posItems and negItems must match in length"))
    return;
  if (require(env, !statsOut || len(env, statsOut) >= 4, "statsOut must hold 4 entries")) return;
  const jsize n = len(env, u);
  Elems e[3];
  const jarray arr[3] = {u, pos, neg};
  const int kind[3] = {kInt, kInt, kInt};
  if (acquire_all(env, e, arr, kind, 3)) return;
  const mf_bpr_params p = bpr_params_of(lr, lambda, 1, scale, 0, 0);
  mf_bpr_stats s = {0, 0, 0, 0};
  int st = mf_bpr_step_triples(CTX(h), &p, n ? (const int32_t*)e[0].p : NULL, n ? (const int32_t*)e[1].p : NULL,
                               n ? (const int32_t*)e[2].p : NULL, n, &s);
  for (int x = 2; x >= 0; --x) release(env, &e[x], JNI_ABORT);
  bpr_finish(env, st, &s, statsOut);
}

JNIEXPORT void JNICALL JFN(bprFit)(JNIEnv* env, jclass c, jlong h, jintArray u, jintArray i, jdouble initScale,
                                   jdouble lr, jdouble lambda, jint batch, jint scale, jint redraws, jlong seed,
                                   jlong steps, jdoubleArray statsOut) {
  if (require(env, u && i && len(env, u) == len(env, i), "users and items must match in length")) return;
  if (require(env, !statsOut || len(env, statsOut) >= 4, "statsOut must hold 4 entries")) return;
  const jsize n = len(env, u);
  Elems e[2];
  const jarray arr[2] = {u, i};
  const int kind[2] = {kInt, kInt};
  if (acquire_all(env, e, arr, kind, 2)) return;
  const mf_bpr_params p = bpr_params_of(lr, lambda, batch, scale, redraws, seed);
  mf_bpr_stats s = {0, 0, 0, 0};
  int st = mf_bpr_fit(CTX(h), n ? (const int32_t*)e[0].p : NULL, n ? (const int32_t*)e[1].p : NULL, n, initScale, &p,
                      steps, &s);
  for (int x = 1; x >= 0; --x) release(env, &e[x], JNI_ABORT);
  bpr_finish(env, st, &s, statsOut);
}

JNIEXPORT void JNICALL JFN(recommendSeen)(JNIEnv* env, jclass c, jlong h, jint side, jintArray q, jint top,
                                          jintArray ids, jdoubleArray scores, jintArray counts) {
  if (require(env, q && ids && counts, "queries, idsOut and countsOut must not be null")) return;
  if (require(env, top >= 1 && top <= MF_RECOMMEND_MAX_TOP, "topN out of range")) return;
  const jsize n = len(env, q);
  if (require(env, (jlong)len(env, ids) >= (jlong)n * top && (!scores || (jlong)len(env, scores) >= (jlong)n * top) &&
                       len(env, counts) >= n,
              "idsOut / scoresOut must hold queries.length * topN entries and countsOut queries.length"))
    return;
  Elems e[4];
  const jarray arr[4] = {q, ids, scores, counts};
  const int kind[4] = {kInt, kInt, kDouble, kInt};
  if (acquire_all(env, e, arr, kind, 4)) return;
  int st = mf_recommend_seen(CTX(h), side, (const int32_t*)e[0].p, n, top, (int32_t*)e[1].p, (double*)e[2].p,
                             (int32_t*)e[3].p);
  for (int x = 3; x >= 1; --x) release(env, &e[x], st == MF_OK ? 0 : JNI_ABORT);
  release(env, &e[0], JNI_ABORT);
  check(env, st);
}

/* the output-array checks recommend, similar and recommendVectors share; 0 when ok */
static int top_lists_fit(JNIEnv* env, jsize n, jint top, jintArray ids, jdoubleArray scores, jintArray counts) {
  if (require(env, ids && counts, "idsOut and countsOut must not be null")) return -1;
  if (require(env, top >= 1 && top <= MF_RECOMMEND_MAX_TOP, "topN out of range")) return -1;
  return require(env, (jlong)len(env, ids) >= (jlong)n * top && (!scores || (jlong)len(env, scores) >= (jlong)n * top) &&
                          len(env, counts) >= n,
                 "idsOut / scoresOut must hold one row of topN entries per query and countsOut one entry");
}

JNIEXPORT void JNICALL JFN(similar)(JNIEnv* env, jclass c, jlong h, jint side, jintArray q, jint top, jint metric,
                                    jboolean self, jintArray xq, jintArray xc, jintArray ids, jdoubleArray scores,
                                    jintArray counts) {
  if (require(env, q != NULL, "queries must not be null")) return;
  const jsize n = len(env, q), ne = xq ? len(env, xq) : 0;
  if (top_lists_fit(env, n, top, ids, scores, counts)) return;
  if (require(env, (!xq && !xc) || (xq && xc && len(env, xq) == len(env, xc)),
              "exclQuery and exclCand must both be null or match in length"))
    return;
  Elems e[6];
  const jarray arr[6] = {q, xq, xc, ids, scores, counts};
  const int kind[6] = {kInt, kInt, kInt, kInt, kDouble, kInt};
  if (acquire_all(env, e, arr, kind, 6)) return;
  int st = mf_similar(CTX(h), side, (const int32_t*)e[0].p, n, top, metric, self ? 1 : 0,
                      ne ? (const int32_t*)e[1].p : NULL, ne ? (const int32_t*)e[2].p : NULL, ne, (int32_t*)e[3].p,
                      (double*)e[4].p, (int32_t*)e[5].p);
  for (int x = 5; x >= 3; --x) release(env, &e[x], st == MF_OK ? 0 : JNI_ABORT);
  for (int x = 2; x >= 0; --x) release(env, &e[x], JNI_ABORT);
  check(env, st);
}

JNIEXPORT void JNICALL JFN(recommendVectors)(JNIEnv* env, jclass c, jlong h, jint side, jdoubleArray vecs, jint n,
                                             jint top, jint metric, jintArray xq, jintArray xc, jintArray ids,
                                             jdoubleArray scores, jintArray counts) {
  const jlong k = rank_of(env, h);
  if (k < 0) return;
  if (require(env, n >= 0 && vecs && (jlong)len(env, vecs) >= (jlong)n * k, "vecs must hold numQueries * k doubles"))
    return;
  if (top_lists_fit(env, n, top, ids, scores, counts)) return;
  if (require(env, (!xq && !xc) || (xq && xc && len(env, xq) == len(env, xc)),
              "exclQueryIndex and exclCand must both be null or match in length"))
    return;
  const jsize ne = xq ? len(env, xq) : 0;
  /* a Java array index is an int; the C call takes 64-bit positions */
  int64_t* xq64 = ne ? (int64_t*)malloc(sizeof(int64_t) * (size_t)ne) : NULL;
  if (require(env, ne == 0 || xq64 != NULL, "out of memory")) return;
  Elems e[6];
  const jarray arr[6] = {vecs, xq, xc, ids, scores, counts};
  const int kind[6] = {kDouble, kInt, kInt, kInt, kDouble, kInt};
  if (acquire_all(env, e, arr, kind, 6)) {
    free(xq64);
    return;
  }
  for (jsize x = 0; x < ne; ++x) xq64[x] = ((const int32_t*)e[1].p)[x];
  int st = mf_recommend_vectors(CTX(h), side, (const double*)e[0].p, n, top, metric, xq64,
                                ne ? (const int32_t*)e[2].p : NULL, ne, (int32_t*)e[3].p, (double*)e[4].p,
                                (int32_t*)e[5].p);
  free(xq64);
  for (int x = 5; x >= 3; --x) release(env, &e[x], st == MF_OK ? 0 : JNI_ABORT);
  for (int x = 2; x >= 0; --x) release(env, &e[x], JNI_ABORT);
  check(env, st);
}

/* A Java array index is an int, so the offsets come as ints; the C call takes 64-bit offsets. */
JNIEXPORT void JNICALL JFN(recommendAmong)(JNIEnv* env, jclass c, jlong h, jint side, jintArray q, jint top,
                                           jintArray off, jintArray cand, jboolean seen, jintArray xq, jintArray xc,
                                           jintArray ids, jdoubleArray scores, jintArray counts) {
  if (require(env, q != NULL && cand != NULL, "queries and candIds must not be null")) return;
  const jsize n = len(env, q), nc = len(env, cand), ne = xq ? len(env, xq) : 0;
  if (top_lists_fit(env, n, top, ids, scores, counts)) return;
  if (require(env, !off || len(env, off) == n + 1, "offsets must be null or hold queries.length + 1 entries")) return;
  if (require(env, (!xq && !xc) || (xq && xc && len(env, xq) == len(env, xc)),
              "exclQuery and exclCand must both be null or match in length"))
    return;
  int64_t* off64 = off ? (int64_t*)malloc(sizeof(int64_t) * ((size_t)n + 1)) : NULL;
  if (require(env, !off || off64 != NULL, "out of memory")) return;
  Elems e[8];
  const jarray arr[8] = {q, off, cand, xq, xc, ids, scores, counts};
  const int kind[8] = {kInt, kInt, kInt, kInt, kInt, kInt, kDouble, kInt};
  if (acquire_all(env, e, arr, kind, 8)) {
    free(off64);
    return;
  }
  for (jsize x = 0; off && x <= n; ++x) off64[x] = ((const int32_t*)e[1].p)[x];
  int st = mf_recommend_among(CTX(h), side, (const int32_t*)e[0].p, n, top, off64, (const int32_t*)e[2].p, nc,
                              seen ? 1 : 0, ne ? (const int32_t*)e[3].p : NULL, ne ? (const int32_t*)e[4].p : NULL, ne,
                              (int32_t*)e[5].p, (double*)e[6].p, (int32_t*)e[7].p);
  free(off64);
  for (int x = 7; x >= 5; --x) release(env, &e[x], st == MF_OK ? 0 : JNI_ABORT);
  for (int x = 4; x >= 0; --x) release(env, &e[x], JNI_ABORT);
  check(env, st);
}

/* Fold-in: mf_als_foldin (rec == 0) / mf_recommend_foldin.  A Java array index is an int, so the offsets come
   as ints; the C call takes 64-bit offsets. */
static void foldin(JNIEnv* env, jlong h, jint side, jintArray off, jintArray cand, jdoubleArray r,
                   const mf_als_solve* how, int rec, jint top, jboolean excl, jintArray ids, jdoubleArray scores,
                   jintArray counts, jdoubleArray vecs, jintArray used) {
  const jlong k = rank_of(env, h);
  if (k < 0) return;
  if (require(env, off && len(env, off) >= 1, "offsets must hold numQueries + 1 entries")) return;
  const jsize n = len(env, off) - 1;
  if (require(env, (!cand && !r) || (cand && r && len(env, cand) == len(env, r)),
              "candIds and ratings must both be null or match in length"))
    return;
  if (require(env, (vecs || rec) && (!vecs || (jlong)len(env, vecs) >= (jlong)n * k), "vecsOut must hold numQueries * k doubles"))
    return;
  if (require(env, !used || len(env, used) >= n, "usedOut must hold one entry per query")) return;
  if (rec && top_lists_fit(env, n, top, ids, scores, counts)) return;
  int64_t* off64 = (int64_t*)malloc(sizeof(int64_t) * ((size_t)n + 1));
  if (require(env, off64 != NULL, "out of memory")) return;
  Elems eo = {0};
  if (acquire(env, &eo, off, kInt)) {
    free(off64);
    return;
  }
  int ok = ((const int32_t*)eo.p)[0] == 0;
  for (jsize x = 0; x <= n; ++x) {
    off64[x] = ((const int32_t*)eo.p)[x];
    if (x > 0 && off64[x] < off64[x - 1]) ok = 0;
  }
  release(env, &eo, JNI_ABORT);
  /* the lists' length against what the C call reads, before any element is touched */
  if (require(env, ok && off64[n] <= (jlong)len(env, cand), "offsets must start at 0, not decrease and end inside candIds")) {
    free(off64);
    return;
  }
  Elems e[7];
  const jarray arr[7] = {cand, r, ids, scores, counts, vecs, used};
  const int kind[7] = {kInt, kDouble, kInt, kDouble, kInt, kDouble, kInt};
  if (acquire_all(env, e, arr, kind, 7)) {
    free(off64);
    return;
  }
  int st = rec ? mf_recommend_foldin(CTX(h), side, off64, (const int32_t*)e[0].p, (const double*)e[1].p, n, how, top,
                                     excl ? 1 : 0, (int32_t*)e[2].p, (double*)e[3].p, (int32_t*)e[4].p, (double*)e[5].p,
                                     (int32_t*)e[6].p)
               : mf_als_foldin(CTX(h), side, off64, (const int32_t*)e[0].p, (const double*)e[1].p, n, how,
                               (double*)e[5].p, (int32_t*)e[6].p);
  free(off64);
  for (int x = 6; x >= 2; --x) release(env, &e[x], st == MF_OK ? 0 : JNI_ABORT);
  for (int x = 1; x >= 0; --x) release(env, &e[x], JNI_ABORT);
  check(env, st);
}

JNIEXPORT void JNICALL JFN(alsFoldin)(JNIEnv* env, jclass c, jlong h, jint side, jintArray off, jintArray cand,
                                      jdoubleArray r, jdouble lambda, jint reg, jint implicit, jdouble alpha,
                                      jint solver, jint cgSteps, jdoubleArray vecs, jintArray used) {
  const mf_als_solve how = als_how(lambda, reg, implicit, alpha, solver, cgSteps);
  foldin(env, h, side, off, cand, r, &how, 0, 0, 0, NULL, NULL, NULL, vecs, used);
}

JNIEXPORT void JNICALL JFN(recommendFoldin)(JNIEnv* env, jclass c, jlong h, jint side, jintArray off, jintArray cand,
                                            jdoubleArray r, jdouble lambda, jint reg, jint implicit, jdouble alpha,
                                            jint solver, jint cgSteps, jint top, jboolean excl, jintArray ids,
                                            jdoubleArray scores, jintArray counts, jdoubleArray vecs, jintArray used) {
  const mf_als_solve how = als_how(lambda, reg, implicit, alpha, solver, cgSteps);
  foldin(env, h, side, off, cand, r, &how, 1, top, excl, ids, scores, counts, vecs, used);
}

JNIEXPORT void JNICALL JFN(rankEvalSeen)(JNIEnv* env, jclass c, jlong h, jint side, jintArray gq, jintArray gc, jint top,
                                         jdoubleArray metrics) {
  if (require(env, gq && gc && len(env, gq) == len(env, gc), "gtQuery and gtCand must match in length")) return;
  if (require(env, metrics && len(env, metrics) >= 8, "metricsOut must hold 8 entries")) return;
  if (require(env, top >= 1 && top <= MF_RECOMMEND_MAX_TOP, "topN out of range")) return;
  const jsize ng = len(env, gq);
  Elems e[3];
  const jarray arr[3] = {gq, gc, metrics};
  const int kind[3] = {kInt, kInt, kDouble};
  if (acquire_all(env, e, arr, kind, 3)) return;
  mf_rank_metrics m;
  int st = mf_rank_eval_seen(CTX(h), side, ng ? (const int32_t*)e[0].p : NULL, ng ? (const int32_t*)e[1].p : NULL, ng,
                             top, &m, NULL, NULL, NULL, 0);
  if (st == MF_OK) {
    double* o = (double*)e[2].p;
    o[0] = (double)m.queries;
    o[1] = (double)m.hits;
    o[2] = m.precision;
    o[3] = m.recall;
    o[4] = m.map;
    o[5] = m.ndcg;
    o[6] = m.mrr;
    o[7] = m.hit_rate;
  }
  release(env, &e[2], st == MF_OK ? 0 : JNI_ABORT);
  for (int x = 1; x >= 0; --x) release(env, &e[x], JNI_ABORT);
  check(env, st);
}

JNIEXPORT void JNICALL JFN(pairRanksSeen)(JNIEnv* env, jclass c, jlong h, jint side, jintArray q, jintArray cd,
                                          jintArray ranks, jintArray valid, jdoubleArray scores) {
  if (require(env, q && cd && len(env, q) == len(env, cd), "queries and cands must match in length")) return;
  const jsize n = len(env, q);
  if (require(env, ranks && len(env, ranks) >= n, "ranksOut must hold one entry per pair")) return;
  if (require(env, (!valid || len(env, valid) >= n) && (!scores || len(env, scores) >= n),
              "validOut / scoresOut must be null or hold one entry per pair"))
    return;
  Elems e[5];
  const jarray arr[5] = {q, cd, ranks, valid, scores};
  const int kind[5] = {kInt, kInt, kInt, kInt, kDouble};
  if (acquire_all(env, e, arr, kind, 5)) return;
  int st = mf_pair_ranks_seen(CTX(h), side, n ? (const int32_t*)e[0].p : NULL, n ? (const int32_t*)e[1].p : NULL, n,
                              (int32_t*)e[2].p, (int32_t*)e[3].p, (double*)e[4].p);
  for (int x = 4; x >= 2; --x) release(env, &e[x], st == MF_OK ? 0 : JNI_ABORT);
  for (int x = 1; x >= 0; --x) release(env, &e[x], JNI_ABORT);
  check(env, st);
}

JNIEXPORT void JNICALL JFN(onlinePrequentialSeen)(JNIEnv* env, jclass c, jlong h, jintArray u, jintArray i,
                                                  jdoubleArray r, jint flavour, jint top, jdoubleArray metrics,
                                                  jintArray ranks, jint negatives, jdouble negRating, jlong seed,
                                                  jlong firstEvent, jintArray sampled, jboolean addEvents) {
  if (require(env, u && i && r && len(env, u) == len(env, i) && len(env, u) == len(env, r),
              "users, items and ratings must match in length"))
    return;
  const jsize n = len(env, u);
  if (require(env, metrics && len(env, metrics) >= 12, "metricsOut must hold 12 entries")) return;
  if (require(env, !ranks || len(env, ranks) >= n, "ranksOut must be null or hold one entry per event")) return;
  if (sampled_shape(env, n, negatives, sampled)) return;
  Elems e[6];
  const jarray arr[6] = {u, i, r, metrics, ranks, sampled};
  const int kind[6] = {kInt, kInt, kDouble, kDouble, kInt, kInt};
  if (acquire_all(env, e, arr, kind, 6)) return;
  mf_prequential m;
  int st = mf_online_prequential_seen(CTX(h), n ? (const int32_t*)e[0].p : NULL, n ? (const int32_t*)e[1].p : NULL,
                                      n ? (const double*)e[2].p : NULL, n, flavour, top, &m, (int32_t*)e[4].p, NULL,
                                      NULL, negatives, negRating, seed, firstEvent, (int32_t*)e[5].p,
                                      addEvents ? 1 : 0);
  if (st == MF_OK) store_prequential((double*)e[3].p, &m);
  for (int x = 5; x >= 3; --x) release(env, &e[x], st == MF_OK ? 0 : JNI_ABORT);
  for (int x = 2; x >= 0; --x) release(env, &e[x], JNI_ABORT);
  check(env, st);
}

typedef int (*eval_fn)(JNIEnv*, jlong, const int32_t*, const int32_t*, const double*, jsize, jdouble, double*);

static int call_rmse(JNIEnv* env, jlong h, const int32_t* u, const int32_t* i, const double* r, jsize n, jdouble unused,
                     double* out) {
  int64_t matched = 0;
  (void)env;
  (void)unused;
  return mf_rmse(CTX(h), u, i, r, n, out, &matched);
}

static int call_risk(JNIEnv* env, jlong h, const int32_t* u, const int32_t* i, const double* r, jsize n, jdouble lambda,
                     double* out) {
  (void)env;
  return mf_empirical_risk(CTX(h), u, i, r, n, lambda, out);
}

static jdouble with_labeled(JNIEnv* env, jlong h, jintArray u, jintArray i, jdoubleArray r, jdouble lambda,
                            eval_fn fn) {
  jsize n = 0;
  if (rating_columns(env, u, i, r, &n)) return 0;
  Elems eu = {0}, ei = {0}, er = {0};
  if (acquire(env, &eu, u, kInt) || acquire(env, &ei, i, kInt) || acquire(env, &er, r, kDouble)) {
    release(env, &ei, JNI_ABORT);
    release(env, &eu, JNI_ABORT);
    return 0;
  }
  double v = 0;
  int st = fn(env, h, (const int32_t*)eu.p, (const int32_t*)ei.p, (const double*)er.p, n, lambda, &v);
  release(env, &er, JNI_ABORT);
  release(env, &ei, JNI_ABORT);
  release(env, &eu, JNI_ABORT);
  check(env, st);
  return v;
}

JNIEXPORT jdouble JNICALL JFN(rmse)(JNIEnv* env, jclass c, jlong h, jintArray u, jintArray i, jdoubleArray r) {
  return with_labeled(env, h, u, i, r, 0.0, call_rmse);
}

JNIEXPORT jdouble JNICALL JFN(empiricalRisk)(JNIEnv* env, jclass c, jlong h, jintArray u, jintArray i,
                                             jdoubleArray r, jdouble lambda) {
  return with_labeled(env, h, u, i, r, lambda, call_risk);
}

JNIEXPORT void JNICALL JFN(blockUpdate)(JNIEnv* env, jclass c, jlong h, jdoubleArray r, jintArray uidx,
                                        jintArray iidx, jdoubleArray users, jintArray uom, jdoubleArray items,
                                        jintArray iom, jint k, jint iteration, jint rbid, jlong seed, jdouble lr,
                                        jint lrm, jdouble lra, jdouble lambda) {
  if (require(env, r && uidx && iidx && users && uom && items && iom, "arguments must not be null")) return;
  const jsize n = len(env, r), nu = len(env, uom), ni = len(env, iom);
  if (require(env, k >= 1 && len(env, uidx) == n && len(env, iidx) == n &&
                       (jlong)len(env, users) >= (jlong)nu * k && (jlong)len(env, items) >= (jlong)ni * k,
              "uidx / iidx must match r in length; users / items must hold omegas.length * k doubles"))
    return;
  Elems er = {0}, eu = {0}, ei = {0}, eU = {0}, eUo = {0}, eI = {0}, eIo = {0};
  Elems* all[7] = {&er, &eu, &ei, &eU, &eUo, &eI, &eIo};
  if (acquire(env, &er, r, kDouble) || acquire(env, &eu, uidx, kInt) || acquire(env, &ei, iidx, kInt) ||
      acquire(env, &eU, users, kDouble) || acquire(env, &eUo, uom, kInt) || acquire(env, &eI, items, kDouble) ||
      acquire(env, &eIo, iom, kInt)) {
    for (int x = 0; x < 7; ++x) release(env, all[x], JNI_ABORT);
    return;
  }
  int st = mf_block_update(CTX(h), (const double*)er.p, (const int32_t*)eu.p, (const int32_t*)ei.p, n, (double*)eU.p,
                           (const int32_t*)eUo.p, nu, (double*)eI.p, (const int32_t*)eIo.p, ni, k, iteration, rbid,
                           seed, lr, lrm, lra, lambda);
  release(env, &eIo, JNI_ABORT);
  release(env, &eI, st == MF_OK ? 0 : JNI_ABORT);
  release(env, &eUo, JNI_ABORT);
  release(env, &eU, st == MF_OK ? 0 : JNI_ABORT);
  release(env, &ei, JNI_ABORT);
  release(env, &eu, JNI_ABORT);
  release(env, &er, JNI_ABORT);
  check(env, st);
}

JNIEXPORT void JNICALL JFN(onlineUpdate)(JNIEnv* env, jclass c, jlong h, jintArray u, jintArray i, jdoubleArray r,
                                         jint flavour, jint parts) {
  jsize n = 0;
  if (rating_columns(env, u, i, r, &n)) return;
  Elems eu = {0}, ei = {0}, er = {0};
  if (acquire(env, &eu, u, kInt) || acquire(env, &ei, i, kInt) || acquire(env, &er, r, kDouble)) {
    release(env, &ei, JNI_ABORT);
    release(env, &eu, JNI_ABORT);
    return;
  }
  int st = mf_online_update(CTX(h), (const int32_t*)eu.p, (const int32_t*)ei.p, (const double*)er.p, n, flavour, parts,
                            NULL, NULL);
  release(env, &er, JNI_ABORT);
  release(env, &ei, JNI_ABORT);
  release(env, &eu, JNI_ABORT);
  check(env, st);
}

JNIEXPORT void JNICALL JFN(onlineUpdateOut)(JNIEnv* env, jclass c, jlong h, jintArray u, jintArray i, jdoubleArray r,
                                            jint flavour, jdoubleArray uout, jdoubleArray iout) {
  jsize n = 0;
  if (rating_columns(env, u, i, r, &n)) return;
  const jlong k = rank_of(env, h);
  if (k < 0) return;
  if (require(env, (!uout || (jlong)len(env, uout) >= (jlong)n * k) && (!iout || (jlong)len(env, iout) >= (jlong)n * k),
              "per-rating output buffers must hold ratings.length * k doubles"))
    return;
  Elems eu = {0}, ei = {0}, er = {0}, euo = {0}, eio = {0};
  if (acquire(env, &eu, u, kInt) || acquire(env, &ei, i, kInt) || acquire(env, &er, r, kDouble) ||
      acquire(env, &euo, uout, kDouble) || acquire(env, &eio, iout, kDouble)) {
    release(env, &euo, JNI_ABORT);
    release(env, &er, JNI_ABORT);
    release(env, &ei, JNI_ABORT);
    release(env, &eu, JNI_ABORT);
    return;
  }
  int st = mf_online_update_out(CTX(h), (const int32_t*)eu.p, (const int32_t*)ei.p, (const double*)er.p, n, flavour, 0,
                                NULL, NULL, (double*)euo.p, (double*)eio.p);
  release(env, &eio, st == MF_OK ? 0 : JNI_ABORT);
  release(env, &euo, st == MF_OK ? 0 : JNI_ABORT);
  release(env, &er, JNI_ABORT);
  release(env, &ei, JNI_ABORT);
  release(env, &eu, JNI_ABORT);
  check(env, st);
}

JNIEXPORT void JNICALL JFN(lookup)(JNIEnv* env, jclass c, jlong h, jint side, jintArray ids, jdoubleArray out,
                                   jbyteArray found) {
  const jlong k = rank_of(env, h);
  if (k < 0) return;
  if (require(env, ids && out && found, "arguments must not be null")) return;
  const jsize n = len(env, ids);
  if (require(env, (jlong)len(env, out) >= (jlong)n * k && len(env, found) >= n,
              "out must hold ids.length * k doubles and found ids.length entries"))
    return;
  Elems ei = {0}, eo = {0}, ef = {0};
  if (acquire(env, &ei, ids, kInt) || acquire(env, &eo, out, kDouble) || acquire(env, &ef, found, kByte)) {
    release(env, &eo, JNI_ABORT);
    release(env, &ei, JNI_ABORT);
    return;
  }
  int st = mf_lookup(CTX(h), side, (const int32_t*)ei.p, n, (double*)eo.p, (uint8_t*)ef.p);
  release(env, &ef, st == MF_OK ? 0 : JNI_ABORT);
  release(env, &eo, st == MF_OK ? 0 : JNI_ABORT);
  release(env, &ei, JNI_ABORT);
  check(env, st);
}

JNIEXPORT jlong JNICALL JFN(countRatings)(JNIEnv* env, jclass c, jstring path, jchar d, jint skip) {
  if (require(env, path != NULL, "path must not be null")) return 0;
  const char* p = (*env)->GetStringUTFChars(env, path, NULL);
  if (!p) return 0;
  int64_t n = 0;
  int st = mf_read_ratings(p, (char)d, skip, NULL, NULL, NULL, 0, &n);
  (*env)->ReleaseStringUTFChars(env, path, p);
  check(env, st);
  return n;
}

JNIEXPORT void JNICALL JFN(readRatings)(JNIEnv* env, jclass c, jstring path, jchar d, jint skip, jintArray u,
                                        jintArray i, jdoubleArray r) {
  if (require(env, path != NULL, "path must not be null")) return;
  jsize cap = 0;
  if (rating_columns(env, u, i, r, &cap)) return;
  Elems eu = {0}, ei = {0}, er = {0};
  if (acquire(env, &eu, u, kInt) || acquire(env, &ei, i, kInt) || acquire(env, &er, r, kDouble)) {
    release(env, &ei, JNI_ABORT);
    release(env, &eu, JNI_ABORT);
    return;
  }
  const char* p = (*env)->GetStringUTFChars(env, path, NULL);
  int64_t n = 0;
  int st = p ? mf_read_ratings(p, (char)d, skip, (int32_t*)eu.p, (int32_t*)ei.p, (double*)er.p, cap, &n) : MF_ERR_INVALID;
  if (p) (*env)->ReleaseStringUTFChars(env, path, p);
  release(env, &er, st == MF_OK ? 0 : JNI_ABORT);
  release(env, &ei, st == MF_OK ? 0 : JNI_ABORT);
  release(env, &eu, st == MF_OK ? 0 : JNI_ABORT);
  if (p) check(env, st);
}

JNIEXPORT void JNICALL JFN(saveModel)(JNIEnv* env, jclass c, jlong h, jstring path) {
  if (require(env, path != NULL, "path must not be null")) return;
  const char* p = (*env)->GetStringUTFChars(env, path, NULL);
  if (!p) return;
  int st = mf_save_model(CTX(h), p);
  (*env)->ReleaseStringUTFChars(env, path, p);
  check(env, st);
}

JNIEXPORT jlong JNICALL JFN(loadModel)(JNIEnv* env, jclass c, jlong h, jstring path) {
  if (require(env, path != NULL, "path must not be null")) return 0;
  const char* p = (*env)->GetStringUTFChars(env, path, NULL);
  if (!p) return 0;
  int64_t step = 0;
  int st = mf_load_model(CTX(h), p, &step);
  (*env)->ReleaseStringUTFChars(env, path, p);
  check(env, st);
  return step;
}
