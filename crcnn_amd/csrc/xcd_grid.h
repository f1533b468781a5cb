// xcd_grid.h -- the grid of a launch whose workgroups are mapped by xcd_group (ntt_device.h): `groups` groups of G workgroups, each group on one of the 8 XCDs.
// No HIP types: the launchers (kernels.h) and the row-transform selector (ntt_select.h) share this one definition.
#pragma once
#include <stddef.h>
static inline unsigned xcd_grid(size_t groups, unsigned G) { return (unsigned)((groups + 7) / 8 * 8 * G); }
