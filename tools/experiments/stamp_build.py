#!/usr/bin/env python3
"""Experiment: where the fixed cost of a short rollout launch goes, and where its waves sit.  Builds build_variants/stamp.so
from a PATCHED COPY of csrc/step_kernel.hip (csrc itself carries no experiment switches): lane 0 of every workgroup reads the
100 MHz real-time counter at kernel entry, behind the initial table fill, behind the step loop and at the end, and leaves the
four low words where ep_sums would go (15 floats per workgroup of 3 environments: 20 x 10 shapes only).  Behind them: the
wave's hardware-id and XCC-id registers (s_getreg: which XCD, shader engine, CU and SIMD it ran on) and the counter at each
quarter of the step loop (the rate of a wave while its CU is full, and after the lone waves beside it have left).
The copy also gets `placement_probe_kernel` with a C entry `uavtrack_stamp_probe`: workgroups of 512 threads that record
the same two registers per wave and stay resident for a bounded time -- where the eight waves of a workgroup that has a CU
to itself sit.  Run tools/experiments/stamp_run.py on the GPU box against the result.
usage: stamp_build.py [--age-balance]   (default: the priority switch `kAgeBalance` of the step loop OFF, the state the recorded
placement figures were taken in; --age-balance: the step loop as csrc has it)"""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
src = os.path.join(ROOT, "marl-uavs-targets-tracking_amd", "csrc")
dst = os.path.join(ROOT, "build_variants", "stamp_src")
os.makedirs(dst, exist_ok=True)
for f in os.listdir(src):
    if f.endswith((".h", ".hip")):
        open(os.path.join(dst, f), "w").write(open(os.path.join(src, f)).read())
p = os.path.join(dst, "step_kernel.hip")
s = open(p).read()


# s_getreg_b32 operands: register id | offset << 6 | (width - 1) << 11, all 32 bits of HW_ID (4) and XCC_ID (20)
HW_ID, XCC_ID = 4 | 31 << 11, 20 | 31 << 11


def once(old, new):
    global s
    assert s.count(old) == 1, (s.count(old), old)
    s = s.replace(old, new)


# The placement figures of DESIGN 4.1.3 (profiles/r06_relay_experiments.txt) are of the step loop WITHOUT the priority switch
# that was built on them: the stamped copy turns it off unless --age-balance asks for the kernel as it ships.
if "--age-balance" not in sys.argv[1:]:
    once("    constexpr bool kAgeBalance = kStepsPerIter == 2 && N_ == 20 && M_ == 10;\n", "    constexpr bool kAgeBalance = false;\n")
once("    StepParams p = p_in;\n", "    const unsigned long long st0 = wall_clock64();\n"
     "    const unsigned st_hw = __builtin_amdgcn_s_getreg(%d), st_xcc = __builtin_amdgcn_s_getreg(%d);\n"
     "    unsigned long long stq1 = 0, stq2 = 0, stq3 = 0;\n    StepParams p = p_in;\n" % (HW_ID, XCC_ID))
once("    for (int t0 = 0; t0 < p.T; t0 += kStepsPerIter) {\n",
     "    for (int t0 = 0; t0 < p.T; t0 += kStepsPerIter) {\n"
     "        { const int tq = (p.T >> 2) & ~1;      // (uniform: scalar compares, three clock reads per launch)\n"
     "          if (tq > 0) { if (t0 == tq) stq1 = wall_clock64(); else if (t0 == 2 * tq) stq2 = wall_clock64(); else if (t0 == 3 * tq) stq3 = wall_clock64(); } }\n")
once("    __syncthreads();\n    if (one_target_per_lane && my_target) {",
     "    __syncthreads();\n    const unsigned long long st1 = wall_clock64();\n    if (one_target_per_lane && my_target) {")
once("    if (kPoolEmit) {                         // what the pool and an uncollected block have left",
     "    const unsigned long long st2 = wall_clock64();\n    if (kPoolEmit) {                         // what the pool and an uncollected block have left")
once("    if (p.ep_sums) {\n        __syncthreads();                       // everyone is done with the tables",
     "    if (p.ep_sums) {\n        const unsigned long long st3 = wall_clock64();\n"
     "        // (nine words: a last workgroup with a single environment owns five and stays silent)\n"
     "        if (tid == 0 && 15 * (size_t)grp + 9 <= 5 * (size_t)p.B) { unsigned *q = reinterpret_cast<unsigned *>(p.ep_sums) + 15 * (size_t)grp; q[0] = (unsigned)st0; q[1] = (unsigned)st1; q[2] = (unsigned)st2; q[3] = (unsigned)st3; "
     "q[4] = st_hw; q[5] = st_xcc; q[6] = (unsigned)stq1; q[7] = (unsigned)stq2; q[8] = (unsigned)stq3; }\n"
     "        return;\n        __syncthreads();                       // everyone is done with the tables")
# the placement probe: no table, no step -- only where the dispatcher puts the waves of a workgroup that cannot share its CU
# (the caller asks for more than half of the CU's LDS).  Every wave spins on the clock for hold_ticks (bounded by an iteration
# count as well) so that the whole grid is resident at once; nothing waits for another wave.
s += """
__global__ void __launch_bounds__(512) placement_probe_kernel(unsigned *out, unsigned hold_ticks)
{
    const unsigned long long t0 = wall_clock64();
    const unsigned hw = __builtin_amdgcn_s_getreg(%d), xcc = __builtin_amdgcn_s_getreg(%d);
    unsigned long long t = t0;
    for (int k = 0; k < 4096 && t - t0 < hold_ticks; ++k) { __builtin_amdgcn_s_sleep(16); t = wall_clock64(); }
    if ((threadIdx.x & 63) == 0) {
        unsigned *q = out + 4 * ((size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
        q[0] = hw; q[1] = xcc; q[2] = (unsigned)t0; q[3] = (unsigned)t;
    }
}

// out: 4 words per wave, blocks * threads / 64 waves.  Returns the hipError_t of the attribute call or the launch.
extern "C" int uavtrack_stamp_probe(unsigned *out, int blocks, int threads, int lds_bytes, unsigned hold_ticks, void *stream)
{
    if (!out || blocks <= 0 || threads < 64 || threads > 512 || threads %% 64 || lds_bytes < 0) return (int)hipErrorInvalidValue;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(placement_probe_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(placement_probe_kernel, dim3(blocks), dim3(threads), (size_t)lds_bytes, static_cast<hipStream_t>(stream), out, hold_ticks);
    return (int)hipGetLastError();
}
""" % (HW_ID, XCC_ID)
open(p, "w").write(s)
out = os.path.join(ROOT, "build_variants", "obj_stamp")
os.makedirs(out, exist_ok=True)
flags = ("--offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-gpu-rdc -ffp-contract=off -I%s/include -I%s -Wno-unused-function -Wno-pass-failed "
         "-fno-convergent-functions -fno-slp-vectorize -mllvm -amdgpu-atomic-optimizer-strategy=None -mllvm -amdgpu-mfma-vgpr-form=1" % (ROOT, dst)).split()
subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["-c", p, "-o", os.path.join(out, "step_kernel.o")], check=True)
# (every object of the library's own build but the patched one: run `make -C csrc` first)
objs = [os.path.join(src, "build", f) for f in sorted(os.listdir(os.path.join(src, "build"))) if f.endswith(".o") and f != "step_kernel.o"] + [os.path.join(out, "step_kernel.o")]
subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-o", os.path.join(ROOT, "build_variants", "stamp.so")] + objs, check=True)
print("built build_variants/stamp.so")
