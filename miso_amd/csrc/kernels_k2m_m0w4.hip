// sampler_k2_multi<0, 4> (kernels_k2m.inl)
// The several-rounds layout of the wide-range batches (se_k2_hg19_defaults) keeps the iteration loop's wave-uniform constants
// as plain scalars (kernels_k2.inl k2_lane_const): this unit is less short of scalar registers than the one-round kernel's,
// and a launch that ends with its largest chains running alone pays the v_readfirstlane's latency, not its issue slot.
// Same sitting, medians of three launches, three runs each: parent 114.49 / 114.19 / 114.21 ms, with the fetches 114.60 /
// 114.89 / 114.68, without 114.08 / 114.04 / 113.98 (profiles/k2_step_scalars.txt).  The recording block and the rest of the
// step are the same text in every unit.
#define MISO_K2_LANE_CONST 0
#include "kernels_k2m.inl"
namespace miso {
template __global__ void sampler_k2_multi<0, 4>(const KernelArgs);
}
