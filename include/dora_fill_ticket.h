/*
 * dora_fill_ticket.h — the ticket a producer's own kernel publishes its sample with.
 *
 * Issued on the host by dora_sample_fill_ticket (dora_gpu.h), passed by value as a kernel
 * argument and consumed on the device by dora_fill_publish (dora_gpu_device.h).  Plain C, the
 * same 32 bytes in C, C++ and HIP device code; both of those headers include this one.
 */
#ifndef DORA_FILL_TICKET_H
#define DORA_FILL_TICKET_H

#include <stdint.h>

/* How the kernel stored the sample (dora_fill_ticket.mode). */
#define DORA_FILL_WRITE_THROUGH 0u /* every sample byte through the dora_st* helpers          */
#define DORA_FILL_PLAIN 1u         /* ordinary stores: each workgroup releases at agent scope */

#define DORA_FILL_MAX_WORKGROUPS 4096u /* done words a fill flag owns */
#define DORA_FILL_TICKET_SIZE 32

typedef struct dora_fill_ticket {
  uint64_t flag;       /* device address of the fill flag's epoch word (start and signal stamps
                          follow it at +8 and +16) */
  uint64_t done;       /* device address of this flag's workgroup done words (uint32_t each) */
  uint64_t epoch;      /* the send epoch the flag is raised to */
  uint32_t workgroups; /* workgroups of the one launch the ticket was issued for */
  uint32_t mode;       /* DORA_FILL_WRITE_THROUGH / DORA_FILL_PLAIN */
} dora_fill_ticket;

#ifdef __cplusplus
static_assert(sizeof(dora_fill_ticket) == DORA_FILL_TICKET_SIZE, "dora_fill_ticket is 32 bytes");
#else
_Static_assert(sizeof(dora_fill_ticket) == DORA_FILL_TICKET_SIZE, "dora_fill_ticket is 32 bytes");
#endif

#endif /* DORA_FILL_TICKET_H */
