// TEST INFRASTRUCTURE ONLY -- Madrona stand-in: the one math type the sim files use.
#pragma once

namespace madrona {
namespace math {

struct Vector2 {
    float x;
    float y;
};

}  // namespace math
}  // namespace madrona
