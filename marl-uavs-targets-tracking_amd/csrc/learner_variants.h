// learner_variants.h -- the ten instantiations of the gradient kernel (learner_kernel.hip) and the rule that picks one.
// No HIP in here: learner_kernel.hip expands the table over its kernels, a host program can expand it over their names.
#pragma once

namespace uavtrack {

// X(kernel, its argument struct, kReg, kTgt, kClip, kAdv, asks for the clipped LDS size: R more floats for log_mu)
#define UAVTRACK_LEARNER_GRAD_VARIANTS(X)                                        \
    X(learner_grad_kernel,                 GradArgs,     0, 0, 0, 0, 0)          \
    X(learner_grad_reg_kernel,             GradArgs,     1, 0, 0, 0, 0)          \
    X(learner_grad_target_kernel,          GradArgs,     0, 1, 0, 0, 0)          \
    X(learner_grad_reg_target_kernel,      GradArgs,     1, 1, 0, 0, 0)          \
    X(learner_grad_clip_kernel,            GradClipArgs, 1, 0, 1, 0, 1)          \
    X(learner_grad_clip_target_kernel,     GradClipArgs, 1, 1, 1, 0, 1)          \
    X(learner_grad_adv_kernel,             GradAdvArgs,  1, 0, 0, 1, 0)          \
    X(learner_grad_adv_target_kernel,      GradAdvArgs,  1, 1, 0, 1, 0)          \
    X(learner_grad_adv_clip_kernel,        GradAdvArgs,  1, 0, 1, 1, 1)          \
    X(learner_grad_adv_clip_target_kernel, GradAdvArgs,  1, 1, 1, 1, 1)

struct LearnerGradVariant {
    const char *kernel;
    bool reg, target, clip, adv, clipped_lds;
};
#define UAVTRACK_VARIANT_ROW(k, Args, reg, tgt, clip, adv, lds) {#k, reg, tgt, clip, adv, lds},
constexpr LearnerGradVariant kLearnerGradVariants[] = {UAVTRACK_LEARNER_GRAD_VARIANTS(UAVTRACK_VARIANT_ROW)};
#undef UAVTRACK_VARIANT_ROW
constexpr int kLearnerGradVariantCount = sizeof(kLearnerGradVariants) / sizeof(kLearnerGradVariants[0]);

// The variant of one launch, as an index into the table: reg = an entropy bonus or an installed entropy buffer,
// target = a target critic is on, log_mu = the batch brings behaviour log-probabilities (the clipped surrogate),
// adv = the advantage mode is not raw.  The clip and the normalised advantage live in the kReg block, so either
// implies it; -1 if the table lacks the entry.
constexpr int learner_grad_variant(bool reg, bool target, bool log_mu, bool adv)
{
    const bool r = reg || log_mu || adv;
    for (int i = 0; i < kLearnerGradVariantCount; ++i) {
        const LearnerGradVariant &v = kLearnerGradVariants[i];
        if (v.reg == r && v.target == target && v.clip == log_mu && v.adv == adv) return i;
    }
    return -1;
}
constexpr bool learner_grad_variants_complete()
{
    for (int f = 0; f < 16; ++f)
        if (learner_grad_variant(f & 1, f & 2, f & 4, f & 8) < 0) return false;
    return true;
}
static_assert(learner_grad_variants_complete(), "every (reg, target, log_mu, adv) has its kernel");

}  // namespace uavtrack
