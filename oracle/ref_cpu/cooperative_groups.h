#include "cuda_on_cpu.h"
