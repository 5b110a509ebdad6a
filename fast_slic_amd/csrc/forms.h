// forms.h -- the record of the kernel forms the dispatch enqueued (testing aid; DESIGN.md, "The form record")
// The assign pass is a family of template instantiations picked by table form, stride, launch size and mode (assign.hip, group.cpp), and
// k_preempt_update has two forms (preempt.hip).  Every launch site notes the code of the instantiation it chose; the process keeps the set
// of distinct codes (fslic_hip_debug_forms_seen) next to the complete list the dispatch can produce (fslic_hip_debug_forms_all, from the
// static tables beside the launch functions).  Host only: one uncontended mutex per launch, nothing on the device.
#pragma once
#include <cstdint>

namespace fslic {

enum : uint32_t { kFormBlk = 1, kFormBin = 2, kFormPre = 3, kFormK32 = 4, kFormGeneric = 5, kFormGenericRec = 6, kFormPreemptUpdate = 7 };
// which spatial table the launch reads: the row-vector table (`tab` in the full pass, `tabs` in a fused one), the full pass's shorter
// 16-row one (`tabv16`), the 2-D table (`tab` / `tabs`), the subsampled stride's 2-D table for 16 rows (`tabs16`), the 32-bit kernel's LUT
enum : uint32_t { kFormTabNone = 0, kFormTabRowvec = 1, kFormTabRowvec16 = 2, kFormTab2d = 3, kFormTab2d16 = 4, kFormTabLut = 5 };

// bits 0-3 family | 4-9 rows per wavefront | 10 fused | 11-13 stride template (0: run-time argument) | 14-16 table | 17 label-free |
// 18 all-pairs (k_preempt_update); _binding.py decodes the same layout
constexpr uint32_t form_code(uint32_t family, int rows, bool fused, int stride_t, uint32_t table, bool nolab = false, bool all_pairs = false) {
    return family | (uint32_t)rows << 4 | (fused ? 1u : 0u) << 10 | (uint32_t)stride_t << 11 | table << 14 | (nolab ? 1u : 0u) << 17 | (all_pairs ? 1u : 0u) << 18;
}

// Adds `code` to the process-wide set (thread-safe).  Called where a launch is enqueued or recorded into a graph; a replay adds nothing.
void note_form(uint32_t code);
// The set so far, at most `cap` codes into `codes`; returns how many there are (-2: more than the record holds).  clear: empty it.
int forms_seen(uint32_t* codes, int cap, bool clear);
// The static tables of every code a launch function can note (assign.hip, preempt.hip)
const uint32_t* assign_forms(int* n);
const uint32_t* preempt_forms(int* n);

}  // namespace fslic
