"""The sensor kernel at every body, sensor, stage and row-source edge, on the device (tests/sensor_cases.py).

Per case, one forward on the device and on the fp64 oracle, then: (a) row counts, types and ids equal the oracle's, the
oracle's qacc and efc_force are written into the Data and mjw.sensor_acc runs on them -- sensordata, cacc, cfrc_int and
cfrc_ext against the oracle at the strict bar, or at 4 x the fp32 oracle's own error where that is larger; (b) on a fresh
Data, fwd_position .. solve, then sensor_pos, sensor_vel and sensor_acc one at a time over a sentinel-filled sensordata:
each writes exactly its stage's slots, bitwise forward's values, and rne_postconstraint gives forward's cacc / cfrc_int /
cfrc_ext; (c) in the batched cases every world is compared with the oracle run of its row; the traced step launches the
expected sensor kernel.

Mutations of csrc/mjw_sensor.hip / mjw_sensor.h that this file turns red (checked by hand, one at a time): skipping the
second chunk of the cacc level pass, flipping `sg` for the second body of a connect / weld, clipping POSITIVE as REAL in
sensor_write, and dropping the sensors with index >= 64 from the acceleration loop."""

import pytest

from tests import sensor_cases as sc


@pytest.mark.gpu
@pytest.mark.parametrize("case", sc.CASES, ids=[c.id for c in sc.CASES])
def test_gpu_sensor_edges(case):
  res = sc.run_case(case)
  print(case.id, res["kernels"], {k: (round(v["device"], 3), round(v["fp32_oracle"], 3), round(v["bar"], 3)) for k, v in res["values"].items()})
  assert not res["failures"], res["failures"]
