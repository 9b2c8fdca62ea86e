// What the HIP double (fake_hip.cc) tells its driver: the live count of every kind of resource, and the fault to inject.
#ifndef FAKE_HIP_H_
#define FAKE_HIP_H_

enum { kFakeDevice = 0, kFakePinned, kFakeEvent, kFakeStream, kFakeGraph, kFakeExec, kFakeKinds };

long fake_hip_live(int kind);          // allocations / handles of that kind handed out and not given back
const char *fake_hip_kind_name(int kind);
long fake_hip_created(void);           // creating calls since the last fake_hip_fail_at
void fake_hip_fail_at(long k);         // the k-th creating call from now fails with hipErrorOutOfMemory (0: none); restarts the count
int fake_hip_fault_hit(void);          // ... and whether it has

#endif
