// nohooks.hip — libcsvgpu.so's side of the link seam: no allocation is ever made to fail (testhooks.hip holds the test build's).
#include "glue.hpp"

namespace csv {
bool test_fail_alloc() { return false; }
}  // namespace csv
