"""Camera parameters for rendering a point cloud -- the reference's utils/pc_to_camera_params.py without Open3D or a window: the
view is fixed (utils/render.default_camera, modelled on Open3D's default view control) instead of picked interactively.

    python -m pcc_geo_cnn_v2_amd.pc_to_camera_params input.ply camera.json [--width 1024 --height 1024 --front 0 0 1 --up 0 1 0
                                                                           --zoom 0.7 --fov 60]

The output is Open3D's PinholeCameraParameters JSON (read by pc_to_img, render_errors and Open3D itself).
"""
import argparse
import logging

from .utils import pc_io, render

logger = logging.getLogger(__name__)


def pc_to_camera_params(input_path, output_path, width=1024, height=1024, front=(0, 0, 1), up=(0, 1, 0), zoom=0.7, fov=60.0):
    cam = render.default_camera(pc_io.load_pc(input_path), width, height, front, up, zoom, fov)
    render.write_camera(output_path, cam)
    logger.info(f'{output_path}: {width}x{height} camera for {input_path}')
    return cam


def main():
    logging.basicConfig(level=logging.INFO, format='%(asctime)s.%(msecs)03d %(levelname)s %(module)s - %(funcName)s: %(message)s',
                        datefmt='%Y-%m-%d %H:%M:%S')
    p = argparse.ArgumentParser(prog='pc_to_camera_params.py', description='Generates camera parameters for a point cloud.',
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('input_path', help='Input point cloud path (ply).')
    p.add_argument('output_path', help='Output camera params path.')
    p.add_argument('--width', type=int, default=1024, help='Image width (new)')
    p.add_argument('--height', type=int, default=1024, help='Image height (new)')
    p.add_argument('--front', type=float, nargs=3, default=(0.0, 0.0, 1.0), help='Direction from the cloud to the camera (new)')
    p.add_argument('--up', type=float, nargs=3, default=(0.0, 1.0, 0.0), help='Up direction of the image (new)')
    p.add_argument('--zoom', type=float, default=0.7, help="Open3D's view zoom (new)")
    p.add_argument('--fov', type=float, default=60.0, help='Vertical field of view in degrees (new)')
    a = p.parse_args()
    pc_to_camera_params(a.input_path, a.output_path, a.width, a.height, a.front, a.up, a.zoom, a.fov)


if __name__ == '__main__':
    main()
