#pragma once
#include "KeyFrame.h"   // TEST INFRASTRUCTURE ONLY (see KeyFrame.h)
