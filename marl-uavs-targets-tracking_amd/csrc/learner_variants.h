// learner_variants.h -- the fourteen instantiations of the gradient kernel (learner_kernel.hip) and the rule that picks one.
// No HIP in here: learner_kernel.hip expands the table over its kernels, a host program can expand it over their names.
#pragma once

namespace uavtrack {

// X(kernel, kReg, kTgt, kClip, kAdv, kStored, lds_extra: floats per tile row behind the common block -- one for log_mu
// with kClip, two for log_mu and the advantage with kStored)
#define UAVTRACK_LEARNER_GRAD_VARIANTS(X)                              \
    X(learner_grad_kernel,                    0, 0, 0, 0, 0, 0)        \
    X(learner_grad_reg_kernel,                1, 0, 0, 0, 0, 0)        \
    X(learner_grad_target_kernel,             0, 1, 0, 0, 0, 0)        \
    X(learner_grad_reg_target_kernel,         1, 1, 0, 0, 0, 0)        \
    X(learner_grad_clip_kernel,               1, 0, 1, 0, 0, 1)        \
    X(learner_grad_clip_target_kernel,        1, 1, 1, 0, 0, 1)        \
    X(learner_grad_adv_kernel,                1, 0, 0, 1, 0, 0)        \
    X(learner_grad_adv_target_kernel,         1, 1, 0, 1, 0, 0)        \
    X(learner_grad_adv_clip_kernel,           1, 0, 1, 1, 0, 1)        \
    X(learner_grad_adv_clip_target_kernel,    1, 1, 1, 1, 0, 1)        \
    X(learner_grad_stored_kernel,             1, 0, 0, 1, 1, 2)        \
    X(learner_grad_stored_target_kernel,      1, 1, 0, 1, 1, 2)        \
    X(learner_grad_stored_clip_kernel,        1, 0, 1, 1, 1, 2)        \
    X(learner_grad_stored_clip_target_kernel, 1, 1, 1, 1, 1, 2)

struct LearnerGradVariant {
    const char *kernel;
    bool reg, target, clip, adv, stored;
    int lds_extra;
};
#define UAVTRACK_VARIANT_ROW(k, reg, tgt, clip, adv, stored, lds) {#k, reg, tgt, clip, adv, stored, lds},
constexpr LearnerGradVariant kLearnerGradVariants[] = {UAVTRACK_LEARNER_GRAD_VARIANTS(UAVTRACK_VARIANT_ROW)};
#undef UAVTRACK_VARIANT_ROW
constexpr int kLearnerGradVariantCount = sizeof(kLearnerGradVariants) / sizeof(kLearnerGradVariants[0]);

// The variant of one launch, as an index into the table: reg = an entropy bonus or an installed entropy buffer,
// target = a target critic is on, log_mu = the batch brings behaviour log-probabilities (the clipped surrogate),
// adv = the advantage mode is not raw, stored = the batch brings stored advantages.  The clip and the normalised
// advantage live in the kReg block, so either implies it; a stored advantage passes through the normalised advantage's
// line (raw being the pair {0, 1}), so it implies both and reg and adv choose nothing.  -1 if the table lacks the entry.
constexpr int learner_grad_variant(bool reg, bool target, bool log_mu, bool adv, bool stored)
{
    const bool a = adv || stored, r = reg || log_mu || a;
    for (int i = 0; i < kLearnerGradVariantCount; ++i) {
        const LearnerGradVariant &v = kLearnerGradVariants[i];
        if (v.reg == r && v.target == target && v.clip == log_mu && v.adv == a && v.stored == stored) return i;
    }
    return -1;
}
constexpr bool learner_grad_variants_complete()
{
    for (int f = 0; f < 32; ++f)
        if (learner_grad_variant(f & 1, f & 2, f & 4, f & 8, f & 16) < 0) return false;
    return true;
}
static_assert(learner_grad_variants_complete(), "every (reg, target, log_mu, adv, stored) has its kernel");

}  // namespace uavtrack
