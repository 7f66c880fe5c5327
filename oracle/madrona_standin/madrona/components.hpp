// TEST INFRASTRUCTURE ONLY -- minimal stand-in for the part of the Madrona engine the reference's
// Hanabi, Cartpole, balance-beam, Overcooked and Simplecooked sim.cpp files use.  Our own code: it holds no game logic.
// Entities, the WorldID column and the Archetype tag.
#pragma once

#include <cstdint>

namespace madrona {

struct Entity {
    uint32_t id;
};

struct WorldID {
    int32_t idx;
};

template <typename... ComponentTs>
struct Archetype {};

}  // namespace madrona
