/* extern "C" entry over the reference's SimpleKNN::knn (simple-knn), compiled for the host (cuda_on_cpu.h). */
#include "cuda_on_cpu.h"

#include "simple_knn.h"

extern "C" void gs4d_ref_knn(int P, const float *points, float *mean_dists) {
    SimpleKNN::knn(P, (float3 *)points, mean_dists);
}
