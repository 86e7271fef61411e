#!/bin/bash
R=${GRAFT_REPO_ROOT:-/root/repo}
cd $R
python3 bench.py --generate-only --no-extras --scene-cache /tmp/sg_scenes 2>/dev/null
python3 bench.py --generate-only --no-extras --seg-profile scannet --scene-cache /tmp/sg_scenes 2>/dev/null
for rep in 1 2; do
for G in 10 12 11; do
  python3 bench.py --full --steps 80 --warmup 10 --repeats 3 --no-cpu-baseline --no-files --no-extras --groups $G --scene-cache /tmp/sg_scenes 2>/dev/null | \
    python3 -c "import json,sys;d=json.loads(sys.stdin.read().strip().splitlines()[-1]);print('voronoi groups $G:',d['repeat_values']['scenes_per_s'])"
done
done
for G in 10 12; do
  python3 bench.py --full --steps 40 --warmup 10 --repeats 3 --no-cpu-baseline --no-files --no-extras --groups $G --seg-profile scannet --scene-cache /tmp/sg_scenes 2>/dev/null | \
    python3 -c "import json,sys;d=json.loads(sys.stdin.read().strip().splitlines()[-1]);print('scannet groups $G:',d['repeat_values']['scenes_per_s'])"
done
