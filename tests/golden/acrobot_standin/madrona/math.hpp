// TEST INFRASTRUCTURE ONLY -- what the reference's Acrobot sim.cpp takes from <madrona/math.hpp>, for
// tests/golden/make_acrobot_golden.py: the include path puts this directory in front of oracle/madrona_standin, whose
// math.hpp has Vector2 alone.  pi is a float, as in Madrona; the vectors are aggregates with operator[].
#pragma once

#include <array>
#include <cstdint>
#include <functional>
#include <vector>

namespace madrona {
namespace math {

constexpr inline float pi = 3.14159265358979323846264338327950288f;

struct Vector2 {
    float x;
    float y;
};

struct Vector3 {
    float x;
    float y;
    float z;
    constexpr float operator[](int i) const { return i == 0 ? x : i == 1 ? y : z; }
};

struct Vector4 {
    float x;
    float y;
    float z;
    float w;
    constexpr float operator[](int i) const { return i == 0 ? x : i == 1 ? y : i == 2 ? z : w; }
};

}  // namespace math
}  // namespace madrona
