/* The radio constants of the simulator's channel model (rl/environment.py, class Environ: Environment.py:48-57 V2V,
 * :127-133 V2I, :183-212), defined ONCE for the host library (csrc/v2xsim.c) and its device counterpart
 * (csrc/v2xsimdev.hip).  tests/test_device_sim_host.py compares them with the Python class. */
#ifndef V2XSIM_CONST_H
#define V2XSIM_CONST_H

#define TWOPI 6.283185307179586476925286766559

static const double V2V_H = 1.5, FC = 2.0, V2V_DECORR = 10.0, V2V_SHADOW_STD = 3.0;
static const double V2I_H_BS = 25.0, V2I_H_MS = 1.5, V2I_DECORR = 50.0, V2I_SHADOW_STD = 8.0;
static const double BS_X = 750.0 / 2, BS_Y = 1299.0 / 2;

#endif /* V2XSIM_CONST_H */
