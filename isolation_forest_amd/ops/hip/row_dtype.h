// Row element type of the input matrix X, as passed to every launch_* in
// forest_kernels.hip. Shared by the kernel TU and its two host callers
// (bindings.cpp, tools/native/ifa_score.cpp).
#pragma once

namespace ifa {

enum RowDtype : int {
  ROW_F32 = 0,   // IEEE binary32
  ROW_BF16 = 1,  // bfloat16 bits (u16 keys, exact <<16 widening)
  ROW_F16 = 2,   // IEEE binary16 bits (u16 keys, exact v_cvt_f32_f16)
};

// bytes per row element
inline int row_elem_bytes(RowDtype dt) { return dt == ROW_F32 ? 4 : 2; }

}  // namespace ifa
