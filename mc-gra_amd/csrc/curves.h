// The third consumer of the two sorted key regions AucRun::finish (auc.hip) leaves behind: the ROC and precision-recall
// curves of mcgra_rank_curves (curves.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mcgra {

// what mcgra_rank_curves was asked for (include/mcgra.h); the roc_* / pr_* triples are device buffers of `cap` entries
struct CurveRequest {
  int drop_intermediate;
  int64_t cap;
  int64_t *roc_tps, *roc_fps;
  float* roc_thr;
  int64_t *pr_tps, *pr_fps;
  float* pr_thr;
  int64_t* counts;      // host[5]
  int64_t* best;        // host[3] or NULL
  float* best_thr;      // host or NULL
};

// keys: the positives' keys ascending at [0, P), the negatives' at [nbase, nbase + N); tmp: a buffer of the same size whose
// contents are free (the sort's second buffer).  Synchronises st.
int rank_curves_sorted(const char* who, hipStream_t st, const uint32_t* keys, uint32_t* tmp, uint64_t P, uint64_t nbase,
                       uint64_t N, const CurveRequest& rq);

}  // namespace mcgra
