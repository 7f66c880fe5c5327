// TEST INFRASTRUCTURE ONLY -- Madrona stand-in: the GPU-backend entry point has no CPU counterpart here;
// the drivers (oracle/ref_driver_*.cpp) create the worlds and run the task graph themselves.
#pragma once

#define MADRONA_BUILD_MWGPU_ENTRY(ContextT, SimT, ConfigT, InitT)
