// learner_variants.h -- the ten instantiations of the gradient kernel (learner_kernel.hip) and the rule that picks one;
// behind them the four of a batch that brings stored advantages, with a table and a rule of their own.
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

// The four instantiations for a batch that brings stored advantages (uavtrack_learner_update_stored / _grad_stored): a
// table and a picker of their own, consulted first when a batch brings them; the ten above are what they were.  Always
// kReg and kAdv (a raw advantage is the pair {0, 1}); the last column asks for the stored LDS size: 2 R more floats, for
// log_mu and the advantage of the tile.
// X(kernel, its argument struct, kReg, kTgt, kClip, kAdv, asks for the stored LDS size)
#define UAVTRACK_LEARNER_STORED_VARIANTS(X)                                         \
    X(learner_grad_stored_kernel,             GradStoredArgs, 1, 0, 0, 1, 1)        \
    X(learner_grad_stored_target_kernel,      GradStoredArgs, 1, 1, 0, 1, 1)        \
    X(learner_grad_stored_clip_kernel,        GradStoredArgs, 1, 0, 1, 1, 1)        \
    X(learner_grad_stored_clip_target_kernel, GradStoredArgs, 1, 1, 1, 1, 1)

#define UAVTRACK_VARIANT_ROW(k, Args, reg, tgt, clip, adv, lds) {#k, reg, tgt, clip, adv, lds},
constexpr LearnerGradVariant kLearnerStoredVariants[] = {UAVTRACK_LEARNER_STORED_VARIANTS(UAVTRACK_VARIANT_ROW)};
#undef UAVTRACK_VARIANT_ROW
constexpr int kLearnerStoredVariantCount = sizeof(kLearnerStoredVariants) / sizeof(kLearnerStoredVariants[0]);

// The stored variant of one launch: target = a target critic is on, log_mu = the batch brings behaviour
// log-probabilities as well.  The entropy term and the advantage mode choose nothing: every stored kernel has both blocks.
constexpr int learner_stored_variant(bool target, bool log_mu)
{
    for (int i = 0; i < kLearnerStoredVariantCount; ++i) {
        const LearnerGradVariant &v = kLearnerStoredVariants[i];
        if (v.reg && v.adv && v.target == target && v.clip == log_mu) return i;
    }
    return -1;
}
static_assert(learner_stored_variant(false, false) >= 0 && learner_stored_variant(true, false) >= 0 &&
              learner_stored_variant(false, true) >= 0 && learner_stored_variant(true, true) >= 0,
              "every (target, log_mu) has its stored kernel");

}  // namespace uavtrack
