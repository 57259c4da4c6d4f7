/* order_sites.h -- TEST-ONLY, force-included in front of qr_host.c by the `order` build (cuda-qr_amd/Makefile): every
 * qrd_stream_wait_event call of the host layer goes to the stub's qrd_stub_wait_at with its site -- the calling function, the text of the
 * event expression and the serial number of the call site in the file (source order) -- so that the wait-removal sweep of
 * tests/test_schedule_order.py can name the wait it skipped without a line number and without an edit of qr_host.c. */
#ifndef ORDER_SITES_H
#define ORDER_SITES_H
#include "../../cuda-qr_amd/csrc/qr_device.h"
int qrd_stub_wait_at(void* s, void* e, const char* func, const char* expr, int site);
#define qrd_stream_wait_event(s, e) qrd_stub_wait_at(s, e, __func__, #e, __COUNTER__)
#endif
