/* units_sites.h -- TEST-ONLY, force-included in front of the host layer's translation units by the `units_*` builds
 * (cuda-qr_amd/Makefile), after the precedent of order_sites.h: every qrd_malloc call of the library goes to the stub's
 * qrd_stub_malloc_at with its site -- the calling function and the text of the pointer expression -- so that the malloc-failure and the
 * shrink sweeps of tests/test_units_stub.py can number the library's own allocations, tell them from the driver's, and name the one they
 * touched without a line number and without an edit of the units. */
#ifndef UNITS_SITES_H
#define UNITS_SITES_H
#include "../../cuda-qr_amd/csrc/qr_device.h"
int qrd_stub_malloc_at(void** p, size_t bytes, const char* func, const char* expr);
#define qrd_malloc(p, bytes) qrd_stub_malloc_at(p, bytes, __func__, #p)
#endif
