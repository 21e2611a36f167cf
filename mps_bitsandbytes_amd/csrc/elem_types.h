// elem_types.h — the two 16-bit element types of every library, device and host code alike.
#pragma once

namespace mbnb {

using f16_t = _Float16;
using bf16_t = __bf16;

}  // namespace mbnb
