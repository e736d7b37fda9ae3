// Host stand-in for ntjoin_amd/csrc/mxg_internal.h, for tools/nthash_check.cpp only: nthash_dev.h takes the variant constants
// of the public header from it and nothing else.
#pragma once
#include "ntjoin_mx.h"
